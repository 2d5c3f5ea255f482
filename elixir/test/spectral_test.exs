defmodule NxSignalAMD.SpectralTest do
  # Spectral.welch/3, csd/4 and coherence/4: Welch's averaged periodogram (scipy.signal.welch / csd / coherence).  The Python suite
  # checks the same kernels against an f64 oracle and scipy's recorded results (tests/test_gpu_welch.py, tests/test_welch_host.py).
  # Not run in the build image (no BEAM); `cd elixir && mix test` on a machine with OTP + a GPU.
  use ExUnit.Case, async: false

  alias NxSignalAMD.Spectral
  alias NxSignalAMD.Windows

  defp rows(shape), do: Nx.iota(shape, type: :f32) |> Nx.multiply(0.37) |> Nx.sin()

  test "shapes and frequencies" do
    x = rows({3, 4096})
    w = Windows.hann(1024)
    {f, pxx} = Spectral.welch(x, w, overlap_length: 768, sampling_rate: 48_000)
    assert Nx.shape(f) == {513} and Nx.shape(pxx) == {3, 513} and Nx.type(pxx) == {:f, 32}
    assert Nx.to_number(f[512]) == 24_000.0
    {_, pxy} = Spectral.csd(x, x, w, fft_length: 2048)
    assert Nx.shape(pxy) == {3, 1025} and Nx.type(pxy) == {:c, 64}
    {_, p255} = Spectral.welch(x, Windows.hann(255))
    assert Nx.shape(p255) == {3, 128}
  end

  test "a sine of amplitude a has a^2 / 2 in its bin of the power spectrum" do
    n = 8192
    t = Nx.iota({n}, type: :f32)
    x = Nx.sin(Nx.multiply(t, 2 * :math.pi() * 64 / 1024)) |> Nx.multiply(3.0)
    {_, p} = Spectral.welch(x, Windows.hann(1024), scaling: :spectrum)
    assert_in_delta Nx.to_number(p[64]), 4.5, 1.0e-3
  end

  test "coherence of a signal with itself is 1, and one frame gives 1" do
    x = rows({2, 5000})
    y = Nx.reverse(x, axes: [1])
    {_, c} = Spectral.coherence(x, x, Windows.hann(512))
    assert Nx.to_number(Nx.reduce_max(Nx.abs(Nx.subtract(c, 1.0)))) <= 1.0e-5
    {_, c1} = Spectral.coherence(Nx.slice_along_axis(x, 0, 512, axis: 1), Nx.slice_along_axis(y, 0, 512, axis: 1), Windows.hann(512))
    assert Nx.to_number(Nx.reduce_max(Nx.abs(Nx.subtract(c1, 1.0)))) <= 1.0e-5
  end

  test "a NaN inside a covered frame poisons its row only" do
    x = rows({3, 2000})
    bad = Nx.indexed_put(x, Nx.tensor([[1, 700]]), Nx.tensor([:nan], type: :f32))
    {_, p} = Spectral.welch(bad, Windows.hann(256))
    {_, clean} = Spectral.welch(x, Windows.hann(256))
    assert Nx.to_number(Nx.all(Nx.is_nan(p[1]))) == 1
    assert p[0] == clean[0] and p[2] == clean[2]
  end

  test "unsupported options are named" do
    x = rows({1000})
    w = Windows.hann(128)
    assert_raise ArgumentError, ~r/detrend :linear is unsupported/, fn -> Spectral.welch(x, w, detrend: :linear) end
    assert_raise ArgumentError, ~r/average :median is unsupported/, fn -> Spectral.welch(x, w, average: :median) end
    assert_raise ArgumentError, ~r/overlap_length/, fn -> Spectral.welch(x, w, overlap_length: 128) end
    assert_raise ArgumentError, ~r/fft_length/, fn -> Spectral.csd(x, x, w, fft_length: 64) end
    assert_raise ArgumentError, ~r/does not fit/, fn -> Spectral.welch(rows({100}), w) end
  end
end
