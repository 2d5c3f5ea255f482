defmodule NxSignalAMD.Filters do
  @moduledoc """
  `NxSignal.Filters.median/2`, `wiener/2` (lib/nx_signal/filters.ex:17-110, :281-303) on the GPU kernels of DESIGN.md section 3.9,
  `firwin/3` (:147-279) and the streaming `fir/3` the reference lacks:
  `fir(x, taps, mode: :same)` == `NxSignal.Convolution.convolve(x, taps, method: :fft, mode: :same)` to fp32
  rounding, computed by overlap-save block FFT convolution on the GPU; `resample_poly/4`, polyphase rational resampling
  (`scipy.signal.resample_poly` with `padtype="constant"`, DESIGN.md section 3.11), which the reference lacks as well.
  """
  alias NxSignalAMD.NIF

  @windows %{hamming: 4, hann: 5, blackman: 3, bartlett: 1, rectangular: 0}
  @modes %{full: 0, same: 1, valid: 2}

  def firwin(num_taps, cutoff, opts \\ []) do
    opts = Keyword.validate!(opts, window: :hamming, pass_zero: true, scale: true, sampling_rate: 2.0, type: {:f, 32})

    if not is_list(cutoff) do
      raise ArgumentError, "cutoff must be a list of frequencies, got: #{inspect(cutoff)}"
    end

    {kind, beta} =
      case opts[:window] do
        {:kaiser, beta} -> {6, beta * 1.0}
        w when is_map_key(@windows, w) -> {@windows[w], 0.0}
        w -> raise ArgumentError, "unknown window #{inspect(w)}, supported: :hamming, :hann, :blackman, :bartlett, :rectangular, {:kaiser, beta}"
      end

    args = [num_taps, Enum.map(cutoff, &(&1 * 1.0)), kind, beta, b(opts[:pass_zero]), b(opts[:scale]), opts[:sampling_rate] * 1.0]

    case Nx.Type.normalize!(opts[:type]) do
      {:f, 64} ->
        {:ok, bin} = apply(NIF, :firwin_f64, args) |> NxSignalAMD.unwrap!()
        Nx.from_binary(bin, :f64)

      {:f, 32} ->
        {:ok, bin} = apply(NIF, :firwin, args) |> NxSignalAMD.unwrap!()
        Nx.from_binary(bin, :f32)

      other ->
        raise ArgumentError, "firwin: type must be {:f, 32} or {:f, 64}, got: #{inspect(other)}"
    end
  end

  def fir(x, taps, opts \\ [])

  # device-resident stream: filtered in HBM, the result stays there
  def fir(%NxSignalAMD.DeviceTensor{type: {:f, 32}} = x, taps, opts) do
    opts = Keyword.validate!(opts, mode: :same)

    if not is_map_key(@modes, opts[:mode]) do
      raise ArgumentError, "expected mode to be one of [:full, :same, :valid], got: #{inspect(opts[:mode])}"
    end

    r = tuple_size(x.shape)
    length = elem(x.shape, r - 1)
    batch_shape = Tuple.delete_at(x.shape, r - 1)
    hb = taps |> Nx.as_type(:f32) |> Nx.to_binary()

    {:ok, yref, n_out} =
      NIF.fir_dev(x.ctx, x.ref, length, Tuple.product(batch_shape), hb, @modes[opts[:mode]]) |> NxSignalAMD.unwrap!()

    %NxSignalAMD.DeviceTensor{ref: yref, ctx: x.ctx, shape: Tuple.insert_at(batch_shape, r - 1, n_out), type: {:f, 32}}
  end

  def fir(x, taps, opts) do
    opts = Keyword.validate!(opts, mode: :same)

    if not is_map_key(@modes, opts[:mode]) do
      raise ArgumentError, "expected mode to be one of [:full, :same, :valid], got: #{inspect(opts[:mode])}"
    end

    shape = Nx.shape(x)
    r = tuple_size(shape)
    length = elem(shape, r - 1)
    batch_shape = Tuple.delete_at(shape, r - 1)
    # f64 operands are transformed in c128 by the reference (convolution.ex:276-284): the f64 tier
    {type, nif, es} =
      if Nx.type(x) == {:f, 64} or Nx.type(taps) == {:f, 64}, do: {:f64, &NIF.fir_f64/6, 8}, else: {:f32, &NIF.fir/6, 4}

    xb = x |> Nx.as_type(type) |> Nx.to_binary()
    hb = taps |> Nx.as_type(type) |> Nx.to_binary()
    {:ok, y} = nif.(NxSignalAMD.context(), xb, length, Tuple.product(batch_shape), hb, @modes[opts[:mode]]) |> NxSignalAMD.unwrap!()
    n_out = div(byte_size(y), es * max(Tuple.product(batch_shape), 1))
    Nx.from_binary(y, type) |> Nx.reshape(Tuple.insert_at(batch_shape, r - 1, n_out))
  end

  @doc """
  Sliding-window median: every output is the median of the `:kernel_shape` window that starts at `min(i, n - k)` on every axis
  (no padding).  The result is f32 of the input's shape; integer tensors are computed like f64.
  """
  def median(t, opts) do
    opts = Keyword.validate!(opts, [:kernel_shape])
    ks = opts[:kernel_shape]

    if not is_tuple(ks) or Nx.rank(t) != tuple_size(ks) do
      raise ArgumentError, message: "kernel shape must be of the same rank as the tensor"
    end

    {type, is_f64} =
      case Nx.type(t) do
        {:c, _} -> raise ArgumentError, "median: complex tensors have no order"
        {:f, 32} -> {:f32, 0}
        _ -> {:f64, 1}
      end

    shape = Tuple.to_list(Nx.shape(t))
    kl = Tuple.to_list(ks)

    Enum.zip(shape, kl)
    |> Enum.each(fn {n, k} ->
      if not (is_integer(k) and k >= 1 and k <= n), do: raise(ArgumentError, "median: kernel_shape #{inspect(ks)} does not fit #{inspect(Nx.shape(t))}")
    end)

    xb = t |> Nx.as_type(type) |> Nx.to_binary()
    {:ok, y} = NIF.median(NxSignalAMD.context(), xb, is_f64, shape, kl) |> NxSignalAMD.unwrap!()
    Nx.from_binary(y, :f32) |> Nx.reshape(Nx.shape(t))
  end

  @doc """
  Wiener filter: local mean and variance over the `:kernel_size` window (mode :same) in f64, `:noise` (nil: the mean local
  variance), the result cast back to the input's type (f32 or f64).
  """
  def wiener(t, opts \\ []) do
    opts = Keyword.validate!(opts, noise: nil, kernel_size: 3)
    rank = Nx.rank(t)

    ks =
      cond do
        is_integer(opts[:kernel_size]) -> Tuple.duplicate(opts[:kernel_size], rank)
        is_tuple(opts[:kernel_size]) -> opts[:kernel_size]
        true -> raise ArgumentError, "kernel_size must be an integer or tuple"
      end

    if tuple_size(ks) != rank do
      raise ArgumentError, "wiener: kernel_size #{inspect(ks)} must have one length per axis of the rank-#{rank} tensor"
    end

    {type, is_f64} =
      case Nx.type(t) do
        {:f, 32} -> {:f32, 0}
        {:f, 64} -> {:f64, 1}
        other -> raise ArgumentError, "wiener: f32 and f64 tensors are built, got: #{inspect(other)}"
      end

    {has_noise, noise} = if is_nil(opts[:noise]), do: {0, 0.0}, else: {1, opts[:noise] * 1.0}
    xb = t |> Nx.to_binary()

    {:ok, y} =
      NIF.wiener(NxSignalAMD.context(), xb, is_f64, Tuple.to_list(Nx.shape(t)), Tuple.to_list(ks), has_noise, noise)
      |> NxSignalAMD.unwrap!()

    Nx.from_binary(y, type) |> Nx.reshape(Nx.shape(t))
  end

  @doc """
  Resamples the last axis of real f32 or complex c64 rows by `up / down` with a polyphase FIR on the GPU, like
  `scipy.signal.resample_poly(x, up, down, padtype="constant")`: `n` samples give `ceil(n * up / down)`.  With the reduced ratio,
  the taps `h` (gain included) and `half = div(length(h) - 1, 2)`: `y[m] = sum_j x[j] * h[m * down + half - j * up]` over the taps
  that exist.  `:window` — any window `firwin/3` takes; the default filter is
  `up * firwin(20 * max(up, down) + 1, [1 / max(up, down)], window: w, sampling_rate: 2.0, type: {:f, 64})` rounded once to f32.
  `:taps` — a 1-D real tensor instead (scipy's array form of `window=`, without the gain: `h = up * taps`).  `up == down` after
  reduction returns the input.  A `DeviceTensor` gives a `DeviceTensor`.  An Inf / NaN sample reaches the outputs whose taps cover
  it and nothing else.
  """
  def resample_poly(x, up, down, opts \\ []) do
    opts = Keyword.validate!(opts, window: {:kaiser, 5.0}, taps: nil, padtype: :constant)

    if not (is_integer(up) and is_integer(down) and up >= 1 and down >= 1) do
      raise ArgumentError, "resample_poly: up and down must be integers >= 1, got: #{inspect(up)}, #{inspect(down)}"
    end

    if opts[:padtype] != :constant do
      raise ArgumentError, "resample_poly: only padtype :constant is built, got: #{inspect(opts[:padtype])}"
    end

    g = Integer.gcd(up, down)
    {up, down} = {div(up, g), div(down, g)}
    hb =
      if up == down and is_nil(opts[:taps]) do
        # no filter is applied, as in scipy: the window is still validated, and one unused tap travels with the call
        firwin(3, [0.5], window: opts[:window])
        <<1.0::float-32-native>>
      else
        resample_taps(up, down, opts[:taps], opts[:window])
      end

    resample_rows(x, up, down, hb)
  end

  defp resample_taps(up, _down, %Nx.Tensor{} = taps, _window) do
    if Nx.rank(taps) != 1 or match?({:c, _}, Nx.type(taps)) do
      raise ArgumentError, "resample_poly: taps must be a 1-D real tensor"
    end

    taps |> Nx.as_type(:f64) |> Nx.multiply(up) |> Nx.as_type(:f32) |> Nx.to_binary()
  end

  defp resample_taps(_up, _down, taps, _window) when not is_nil(taps) do
    raise ArgumentError, "resample_poly: taps must be a 1-D real tensor, got: #{inspect(taps)}"
  end

  defp resample_taps(up, down, nil, window) do
    big = max(up, down)

    firwin(20 * big + 1, [1.0 / big], window: window, sampling_rate: 2.0, type: {:f, 64})
    |> Nx.multiply(up)
    |> Nx.as_type(:f32)
    |> Nx.to_binary()
  end

  defp resample_rows(%NxSignalAMD.DeviceTensor{type: type} = x, up, down, hb) do
    r = tuple_size(x.shape)
    length = elem(x.shape, r - 1)
    batch_shape = Tuple.delete_at(x.shape, r - 1)
    is_complex = if type == {:c, 64}, do: 1, else: 0

    {:ok, yref, n_out} =
      NIF.resample_poly_dev(x.ctx, x.ref, is_complex, length, Tuple.product(batch_shape), hb, up, down) |> NxSignalAMD.unwrap!()

    %NxSignalAMD.DeviceTensor{ref: yref, ctx: x.ctx, shape: Tuple.insert_at(batch_shape, r - 1, n_out), type: type}
  end

  defp resample_rows(x, up, down, hb) do
    {type, is_complex} =
      case Nx.type(x) do
        {:f, 32} -> {:f32, 0}
        {:c, 64} -> {:c64, 1}
        other -> raise ArgumentError, "resample_poly: f32 and c64 tensors are built, got: #{inspect(other)}"
      end

    shape = Nx.shape(x)
    r = tuple_size(shape)
    if r < 1, do: raise(ArgumentError, "resample_poly: the tensor must have at least one axis")
    length = elem(shape, r - 1)
    batch_shape = Tuple.delete_at(shape, r - 1)

    {:ok, y, n_out} =
      NIF.resample_poly(NxSignalAMD.context(), Nx.to_binary(x), is_complex, length, Tuple.product(batch_shape), hb, up, down)
      |> NxSignalAMD.unwrap!()

    Nx.from_binary(y, type) |> Nx.reshape(Tuple.insert_at(batch_shape, r - 1, n_out))
  end

  defp b(true), do: 1
  defp b(_), do: 0
end
