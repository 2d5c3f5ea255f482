defmodule NxSignalAMD.Spectral do
  @moduledoc """
  Spectral estimation on the GPU, which the reference lacks: Welch's averaged periodogram `welch/3`, the cross spectral density
  `csd/4` and the magnitude-squared coherence `coherence/4` of real f32 rows — `scipy.signal.welch / csd / coherence` with
  `return_onesided=True` and `average="mean"` (DESIGN.md section 3.12; include/nxsig.h: `nxsig_welch_f32`, `nxsig_csd_f32`).

  The window is a 1-D tensor of `N` samples, as in `NxSignalAMD.stft/3`.  Options: `:overlap_length` (default `div(N, 2)`),
  `:fft_length` (an integer `>= N` or `:power_of_two`, default `N`), `:sampling_rate` (1.0), `:detrend` (`:constant` or `false`),
  `:scaling` (`:density` or `:spectrum`), `:average` (`:mean`).  Frame `m` covers samples `[m * hop, m * hop + N)`; there is no
  padding and a ragged tail is dropped.  Every function returns `{frequencies, estimate}` with `fft_length / 2 + 1` bins on the last
  axis.  A row (for `csd` and `coherence`: the pair of rows) with an Inf / NaN inside the samples its frames cover is NaN in every bin.
  """
  alias NxSignalAMD.NIF

  @scalings %{density: 0, spectrum: 1}

  @doc "`{f, pxx}`: the power spectral density (`scaling: :density`) or power spectrum (`:spectrum`) of the last axis, f32"
  def welch(x, window, opts \\ []) do
    {n, hop, k, fs, detrend, scaling} = options("welch", window, opts)
    {xb, length, batch_shape} = rows("welch", x, n)

    {:ok, pxx, bins} =
      NIF.welch(NxSignalAMD.context(), xb, length, Tuple.product(batch_shape), wbin(window), hop, k, detrend, scaling, fs)
      |> NxSignalAMD.unwrap!()

    {frequencies(k, fs), Nx.from_binary(pxx, :f32) |> Nx.reshape(out_shape(batch_shape, bins))}
  end

  @doc "`{f, pxy}`: the cross spectral density `mean_m conj(X_m) * Y_m` of two tensors of one shape, c64"
  def csd(x, y, window, opts \\ []) do
    {f, pxy, _pxx, _pyy} = estimate("csd", x, y, window, opts)
    {f, pxy}
  end

  @doc "`{f, cxy}`: `|pxy|^2 / (pxx * pyy)`, f32 in [0, 1], from one `csd` call that also returns both auto-spectra; one frame gives 1"
  def coherence(x, y, window, opts \\ []) do
    {f, pxy, pxx, pyy} = estimate("coherence", x, y, window, opts)
    num = pxy |> Nx.abs() |> Nx.as_type(:f64) |> Nx.pow(2)
    den = Nx.multiply(Nx.as_type(pxx, :f64), Nx.as_type(pyy, :f64))
    {f, Nx.divide(num, den) |> Nx.as_type(:f32)}
  end

  defp estimate(fun, x, y, window, opts) do
    {n, hop, k, fs, detrend, scaling} = options(fun, window, opts)
    {xb, length, batch_shape} = rows(fun, x, n)
    {yb, ^length, ^batch_shape} = rows(fun, y, n)

    {:ok, pxy, pxx, pyy, bins} =
      NIF.csd(NxSignalAMD.context(), xb, yb, length, Tuple.product(batch_shape), wbin(window), hop, k, detrend, scaling, fs)
      |> NxSignalAMD.unwrap!()

    shape = out_shape(batch_shape, bins)

    {frequencies(k, fs), Nx.from_binary(pxy, :c64) |> Nx.reshape(shape), Nx.from_binary(pxx, :f32) |> Nx.reshape(shape),
     Nx.from_binary(pyy, :f32) |> Nx.reshape(shape)}
  end

  defp options(fun, window, opts) do
    if Nx.rank(window) != 1, do: raise(ArgumentError, "#{fun}: the window must be a 1-D tensor")
    n = Nx.size(window)

    opts =
      Keyword.validate!(opts, overlap_length: div(n, 2), fft_length: n, sampling_rate: 1.0, detrend: :constant, scaling: :density, average: :mean)

    overlap = opts[:overlap_length]

    if not (is_integer(overlap) and overlap >= 0 and overlap < n) do
      raise ArgumentError, "#{fun}: overlap_length must be an integer in [0, #{n}), got: #{inspect(overlap)}"
    end

    k =
      case opts[:fft_length] do
        :power_of_two -> next_pow2(n, 1)
        k when is_integer(k) and k >= n -> k
        other -> raise ArgumentError, "#{fun}: fft_length must be an integer >= the window length #{n} or :power_of_two, got: #{inspect(other)}"
      end

    detrend =
      case opts[:detrend] do
        :constant -> 1
        false -> 0
        :linear -> raise ArgumentError, "#{fun}: detrend :linear is unsupported, only :constant and false are built"
        other -> raise ArgumentError, "#{fun}: detrend must be :constant or false, got: #{inspect(other)}"
      end

    if not is_map_key(@scalings, opts[:scaling]) do
      raise ArgumentError, "#{fun}: scaling must be :density or :spectrum, got: #{inspect(opts[:scaling])}"
    end

    if opts[:average] != :mean do
      raise ArgumentError, "#{fun}: average #{inspect(opts[:average])} is unsupported, only :mean is built"
    end

    fs = opts[:sampling_rate]

    if not (is_number(fs) and fs > 0) do
      raise ArgumentError, "#{fun}: sampling_rate must be a positive number, got: #{inspect(fs)}"
    end

    {n, n - overlap, k, fs * 1.0, detrend, @scalings[opts[:scaling]]}
  end

  defp rows(fun, x, n) do
    if Nx.type(x) != {:f, 32}, do: raise(ArgumentError, "#{fun}: real f32 tensors are built, got: #{inspect(Nx.type(x))}")
    shape = Nx.shape(x)
    r = tuple_size(shape)
    if r < 1, do: raise(ArgumentError, "#{fun}: the tensor must have at least one axis")
    length = elem(shape, r - 1)
    if length < n, do: raise(ArgumentError, "#{fun}: the window of length #{n} does not fit rows of length #{length}")
    {Nx.to_binary(x), length, Tuple.delete_at(shape, r - 1)}
  end

  defp wbin(window), do: window |> Nx.as_type(:f32) |> Nx.to_binary()
  defp out_shape(batch_shape, bins), do: Tuple.insert_at(batch_shape, tuple_size(batch_shape), bins)
  defp frequencies(k, fs), do: Nx.iota({div(k, 2) + 1}, type: :f64) |> Nx.multiply(fs / k) |> Nx.as_type(:f32)
  defp next_pow2(n, p) when p >= n, do: p
  defp next_pow2(n, p), do: next_pow2(n, 2 * p)
end
