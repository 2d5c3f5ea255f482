defmodule NxSignalAMD.ResamplePolyTest do
  # Filters.resample_poly/4: polyphase rational resampling (scipy.signal.resample_poly with padtype="constant") of host tensors and
  # DeviceTensors.  The Python suite checks the same kernels against an f64 oracle and scipy's recorded results
  # (tests/test_gpu_resample.py, tests/test_resample_host.py).  Not run in the build image (no BEAM); `cd elixir && mix test` on a
  # machine with OTP + a GPU.
  use ExUnit.Case, async: false

  alias NxSignalAMD, as: Sig
  alias NxSignalAMD.DeviceTensor
  alias NxSignalAMD.Filters

  defp rows(shape), do: Nx.iota(shape, type: :f32) |> Nx.multiply(0.37) |> Nx.sin()

  test "output lengths and the identity" do
    x = rows({3, 1000})
    assert Nx.shape(Filters.resample_poly(x, 1, 3)) == {3, 334}
    assert Nx.shape(Filters.resample_poly(x, 3, 2)) == {3, 1500}
    assert Nx.shape(Filters.resample_poly(x, 160, 441)) == {3, 363}
    assert Filters.resample_poly(x, 5, 5) == x
    assert Filters.resample_poly(x, 5, 5, taps: Nx.tensor([0.25, 0.5])) == x
    assert_raise ArgumentError, ~r/unknown window/, fn -> Filters.resample_poly(x, 5, 5, window: :boxcar) end
    assert Filters.resample_poly(x, 4, 6) == Filters.resample_poly(x, 2, 3)
  end

  test "one tap at 1 / 2 keeps every second sample" do
    x = rows({2, 2051})
    y = Filters.resample_poly(x, 1, 2, taps: Nx.tensor([1.0]))
    assert y == Nx.slice_along_axis(x, 0, 2051, axis: 1, strides: 2)
  end

  test "the definition, term by term, for explicit taps" do
    x = rows({40})
    taps = Nx.tensor([0.25, 0.5, -0.125, 1.0, 0.75])
    y = Filters.resample_poly(x, 3, 4, taps: taps) |> Nx.to_flat_list()
    h = Nx.multiply(taps, 3) |> Nx.to_flat_list()
    xs = Nx.to_flat_list(x)
    assert length(y) == 30

    for {got, m} <- Enum.with_index(y) do
      want =
        for j <- 0..39, i = m * 4 + 2 - j * 3, i >= 0 and i < 5, reduce: 0.0 do
          acc -> acc + Enum.at(xs, j) * Enum.at(h, i)
        end

      assert_in_delta got, want, 1.0e-5
    end
  end

  test "complex rows are their two planes" do
    re = rows({2, 1500})
    im = rows({2, 1500}) |> Nx.cos()
    y = Filters.resample_poly(Nx.complex(re, im), 3, 2)
    assert Nx.type(y) == {:c, 64}
    assert Nx.real(y) == Filters.resample_poly(re, 3, 2)
    assert Nx.imag(y) == Filters.resample_poly(im, 3, 2)
  end

  test "a DeviceTensor gives a DeviceTensor with the same bits and names the kernel" do
    x = rows({3, 48_000})
    xd = DeviceTensor.to_device(x)
    yd = Filters.resample_poly(xd, 1, 3)
    assert %DeviceTensor{type: {:f, 32}, shape: {3, 16_000}} = yd
    assert Sig.last_dispatch(xd.ctx) == "resample.poly.lds"
    assert DeviceTensor.from_device(yd) == Filters.resample_poly(x, 1, 3)
    assert DeviceTensor.from_device(xd) == x
    long = Nx.iota({20_001}, type: :f32) |> Nx.cos() |> Nx.divide(100)
    Filters.resample_poly(xd, 3, 2, taps: long)
    assert Sig.last_dispatch(xd.ctx) == "resample.poly.generic"
  end

  test "argument errors" do
    x = rows({2, 100})
    assert_raise ArgumentError, ~r/up and down/, fn -> Filters.resample_poly(x, 0, 3) end
    assert_raise ArgumentError, ~r/up and down/, fn -> Filters.resample_poly(x, 1, -3) end
    assert_raise ArgumentError, ~r/padtype/, fn -> Filters.resample_poly(x, 1, 3, padtype: :line) end
    assert_raise ArgumentError, ~r/1-D real/, fn -> Filters.resample_poly(x, 1, 3, taps: rows({2, 2})) end
    assert_raise ArgumentError, ~r/f32 and c64/, fn -> Filters.resample_poly(Nx.as_type(x, :f64), 1, 3) end
    assert_raise ArgumentError, ~r/unknown window/, fn -> Filters.resample_poly(x, 1, 3, window: :boxcar) end
    assert_raise ArgumentError, fn -> Filters.resample_poly(x, 1, 3, beta: 5.0) end
  end
end
