defmodule NxSignalAMD.IstftMaskedTest do
  # istft_masked/4 and spectrum_mask/2: time-frequency masks (f32 full, f32 one-sided, c64), broadcast rows, host tensors and
  # DeviceTensors.  The Python suite checks the same calls through the NIF harness (tests/test_gpu_istft_masked.py).  Not run in
  # the build image (no BEAM); `cd elixir && mix test` on a machine with OTP + a GPU.
  use ExUnit.Case, async: false

  alias NxSignalAMD, as: Sig
  alias NxSignalAMD.DeviceTensor

  @opts [overlap_length: 768, sampling_rate: 48_000]

  defp spectrum(shape), do: Nx.iota(shape, type: :f32) |> Nx.sin() |> Nx.as_type(:c64)
  defp gains(shape), do: Nx.iota(shape, type: :f32) |> Nx.cos() |> Nx.abs()

  # the full mask a one-sided one stands for: bin k > K/2 takes mask[K - k]
  defp mirrored(mask, k) do
    idx = Nx.tensor(for i <- 0..(k - 1), do: if(i <= div(k, 2), do: i, else: k - i))
    Nx.take(mask, idx, axis: -1)
  end

  test "a real mask: istft_masked equals multiply-then-istft, fused (N = 1024) and two-step (N = 512)" do
    for {n, overlap} <- [{1024, 768}, {512, 384}] do
      z = spectrum({2, 9, n})
      m = gains({2, 9, n})
      w = Sig.Windows.hann(n)
      opts = [overlap_length: overlap, sampling_rate: 48_000]
      masked = Sig.spectrum_mask(z, m)
      assert Nx.shape(masked) == {2, 9, n}
      # a real gain multiplies each component on its own
      assert masked == Nx.complex(Nx.multiply(Nx.real(z), m), Nx.multiply(Nx.imag(z), m))
      assert Sig.istft_masked(z, m, w, opts) == Sig.istft(masked, w, opts)
    end
  end

  test "a complex mask multiplies like Nx.multiply" do
    z = spectrum({2, 9, 1024})
    m = spectrum({2, 9, 1024}) |> Nx.conjugate()
    w = Sig.Windows.hann(1024)
    assert Sig.spectrum_mask(z, m) == Nx.multiply(z, m)
    assert Sig.istft_masked(z, m, w, @opts) == Sig.istft(Nx.multiply(z, m), w, @opts)
  end

  test "a one-sided mask equals its Hermitian mirror" do
    z = spectrum({2, 9, 1024})
    m = gains({2, 9, 513})
    w = Sig.Windows.hann(1024)
    assert Sig.spectrum_mask(z, m) == Sig.spectrum_mask(z, mirrored(m, 1024))
    assert Sig.istft_masked(z, m, w, @opts) == Sig.istft_masked(z, mirrored(m, 1024), w, @opts)
  end

  test "one mixture and three masks; three spectra and one mask" do
    w = Sig.Windows.hann(1024)
    z1 = spectrum({9, 1024})
    m3 = gains({3, 9, 1024})
    y = Sig.istft_masked(z1, m3, w, @opts)
    assert Nx.shape(y) == {3, 9 * 256 + 768}
    assert y == Sig.istft_masked(Nx.broadcast(z1, {3, 9, 1024}), m3, w, @opts)
    z3 = spectrum({3, 1, 9, 1024})
    m1 = gains({9, 1024})
    y = Sig.istft_masked(z3, m1, w, @opts)
    assert Nx.shape(y) == {3, 1, 9 * 256 + 768}
    assert y == Sig.istft_masked(z3, Nx.broadcast(m1, {3, 1, 9, 1024}), w, @opts)
  end

  test "device-resident operands give a DeviceTensor with the same bits and name the fused kernel" do
    z = spectrum({2, 9, 1024})
    m = gains({2, 9, 513})
    w = Sig.Windows.hann(1024)
    zd = DeviceTensor.to_device(z)
    md = DeviceTensor.to_device(m)
    yd = Sig.istft_masked(zd, md, w, @opts)
    assert %DeviceTensor{type: {:c, 64}, shape: {2, 3072}} = yd
    assert String.starts_with?(Sig.last_dispatch(zd.ctx), "istft.wave.mask")
    assert DeviceTensor.from_device(yd) == Sig.istft_masked(z, m, w, @opts)
    assert DeviceTensor.from_device(Sig.spectrum_mask(zd, md)) == Sig.spectrum_mask(z, m)
    # the operands are left as they were
    assert DeviceTensor.from_device(zd) == z
  end

  test "shape, type, placement and option errors" do
    z = spectrum({2, 9, 1024})
    w = Sig.Windows.hann(1024)
    assert_raise ArgumentError, ~r/frames/, fn -> Sig.istft_masked(z, gains({2, 8, 1024}), w, @opts) end
    assert_raise ArgumentError, ~r/last axis/, fn -> Sig.istft_masked(z, gains({2, 9, 512}), w, @opts) end
    assert_raise ArgumentError, ~r/one-sided mask must be real/, fn -> Sig.istft_masked(z, spectrum({2, 9, 513}), w, @opts) end
    assert_raise ArgumentError, ~r/rows/, fn -> Sig.istft_masked(z, gains({3, 9, 1024}), w, @opts) end
    assert_raise ArgumentError, ~r/even fft_length/, fn -> Sig.spectrum_mask(spectrum({2, 9, 15}), gains({2, 9, 8})) end
    assert_raise ArgumentError, ~r/f64/, fn -> Sig.istft_masked(z, Nx.as_type(gains({2, 9, 1024}), :f64), w, @opts) end
    assert_raise ArgumentError, ~r/f64 window/, fn -> Sig.istft_masked(z, gains({2, 9, 1024}), Nx.as_type(w, :f64), @opts) end
    assert_raise ArgumentError, fn -> Sig.istft_masked(z, gains({2, 9, 1024}), w, window_padding: :valid) end
    assert_raise ArgumentError, ~r/sampling_rate is mandatory/, fn -> Sig.istft_masked(z, gains({2, 9, 1024}), w, scaling: :psd, sampling_rate: nil) end
    assert_raise ArgumentError, ~r/both/, fn -> Sig.istft_masked(DeviceTensor.to_device(z), gains({2, 9, 1024}), w, @opts) end
  end
end
