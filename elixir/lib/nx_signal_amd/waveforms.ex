defmodule NxSignalAMD.Waveforms do
  @moduledoc """
  `NxSignal.Waveforms` (lib/nx_signal/waveforms.ex) for host tensors: `sawtooth/2`, `square/2`, `gaussian_pulse/2`, `chirp/5`,
  `polynomial_sweep/3` and `unit_impulse/2` on the GPU kernels of DESIGN.md section 3.10, and `sinc/1` on the library's host numerics
  (the building block of `Filters.firwin/3`).

  The reference's option names, defaults and ArgumentErrors. An f64 tensor is evaluated in double and gives f64; every other real
  type is read as f32 and reproduces the reference's f32 values bit for bit. `unit_impulse/2` builds f32, f64, s32, s64, u32 and u64
  tensors, refuses narrower types, and raises ArgumentError for an index outside the shape (a deliberate deviation: the reference
  leaves that to `Nx.indexed_put/3`).
  """
  alias NxSignalAMD.NIF

  @methods %{linear: 0, quadratic: 1, logarithmic: 2, hyperbolic: 3}
  @dtypes %{{:f, 32} => 0, {:f, 64} => 1, {:s, 32} => 2, {:s, 64} => 3, {:u, 32} => 4, {:u, 64} => 5}

  @doc "See `NxSignal.Waveforms.sinc/1`. Returns an f32 tensor of the input's shape (f64 for an f64 tensor)."
  def sinc(%Nx.Tensor{type: {:f, 64}} = t) do
    {:ok, out} = NIF.sinc_f64(Nx.to_binary(t)) |> NxSignalAMD.unwrap!()
    Nx.from_binary(out, :f64) |> Nx.reshape(Nx.shape(t))
  end

  def sinc(%Nx.Tensor{} = t) do
    shape = Nx.shape(t)
    {:ok, out} = NIF.sinc(t |> Nx.as_type(:f32) |> Nx.to_binary()) |> NxSignalAMD.unwrap!()
    Nx.from_binary(out, :f32) |> Nx.reshape(shape)
  end

  def sinc(number) when is_number(number), do: sinc(Nx.tensor(number, type: :f32))

  @doc "See `NxSignal.Waveforms.sawtooth/2`. Option `:width` (default 1) in [0, 1]."
  def sawtooth(t, opts \\ []) do
    opts = Keyword.validate!(opts, width: 1)
    width = opts[:width]

    if not is_number(width) or width < 0 or width > 1 do
      raise ArgumentError, "width must be between 0 and 1, inclusive. Got: #{inspect(width)}"
    end

    {bin, f64, type, shape} = input!(t, "sawtooth")
    {:ok, out} = NIF.sawtooth(NxSignalAMD.context(), bin, f64, width) |> NxSignalAMD.unwrap!()
    tensor(out, type, shape)
  end

  @doc "See `NxSignal.Waveforms.square/2`. Option `:duty` (default 0.5): a number or a tensor of `t`'s shape. Returns s32."
  def square(t, opts \\ []) do
    opts = Keyword.validate!(opts, duty: 0.5)
    {bin, f64, type, shape} = input!(t, "square")

    {duty, duty_bin} =
      case opts[:duty] do
        d when is_number(d) ->
          {d, <<>>}

        d ->
          d = Nx.to_tensor(d)

          if Nx.shape(d) != shape do
            raise ArgumentError, "square: duty must have t's shape #{inspect(shape)}, got #{inspect(Nx.shape(d))}"
          end

          {0.0, d |> Nx.as_type(type) |> Nx.to_binary()}
      end

    {:ok, out} = NIF.square(NxSignalAMD.context(), bin, f64, duty, duty_bin) |> NxSignalAMD.unwrap!()
    tensor(out, {:s, 32}, shape)
  end

  @doc """
  See `NxSignal.Waveforms.gaussian_pulse/2`. Options `:center_frequency` (1000), `:bandwidth` (0.5), `:bandwidth_reference_level`
  (-6). Returns `%{envelope: _, in_phase: _, quadrature: _}`.
  """
  def gaussian_pulse(t, opts \\ []) do
    opts = Keyword.validate!(opts, center_frequency: 1000, bandwidth: 0.5, bandwidth_reference_level: -6)
    fc = opts[:center_frequency]
    bw = opts[:bandwidth]
    bwr = opts[:bandwidth_reference_level]

    if not is_number(fc) or fc < 0 do
      raise ArgumentError, "Center frequency must be greater than or equal to 0, got: #{inspect(fc)}"
    end

    if not is_number(bw) or bw <= 0 do
      raise ArgumentError, "Bandwidth must be greater than 0, got: #{inspect(bw)}"
    end

    if not is_number(bwr) or bwr >= 0 do
      raise ArgumentError, "Bandwidth reference level must be less than 0, got: #{inspect(bwr)}"
    end

    {bin, f64, type, shape} = input!(t, "gaussian_pulse")
    {:ok, env, yi, yq} = NIF.gaussian_pulse(NxSignalAMD.context(), bin, f64, fc, bw, bwr) |> NxSignalAMD.unwrap!()
    %{envelope: tensor(env, type, shape), in_phase: tensor(yi, type, shape), quadrature: tensor(yq, type, shape)}
  end

  @doc """
  See `NxSignal.Waveforms.chirp/5`. Options `:phi` (0), `:vertex_zero` (true) and `:method` (`:linear`, `:quadratic`, `:logarithmic`
  or `:hyperbolic`).
  """
  def chirp(t, f0, t1, f1, opts \\ []) do
    opts = Keyword.validate!(opts, phi: 0, vertex_zero: true, method: :linear)
    method = Map.get(@methods, opts[:method])

    if method == nil do
      raise ArgumentError, "invalid method, must be one of #{inspect([:linear, :quadratic, :logarithmic, :hyperbolic])}, got: #{inspect(opts[:method])}"
    end

    if not (is_number(f0) and is_number(t1) and is_number(f1) and is_number(opts[:phi])) do
      raise ArgumentError, "chirp: f0, t1, f1 and :phi must be numbers"
    end

    {bin, f64, type, shape} = input!(t, "chirp")
    vertex_zero = if opts[:vertex_zero] == true, do: 1, else: 0
    {:ok, out} = NIF.chirp(NxSignalAMD.context(), bin, f64, {f0, t1, f1}, method, vertex_zero, opts[:phi]) |> NxSignalAMD.unwrap!()
    tensor(out, type, shape)
  end

  @doc """
  See `NxSignal.Waveforms.polynomial_sweep/3`. `t` and `coefs` are rank 1, `coefs` with 1 to 32 entries from the highest power down.
  Options `:phi` (0) and `:phi_unit` (`:radians` or `:degrees`). The dot product of the integrated coefficients with the powers of
  `t` is summed in f64 and rounded once.
  """
  def polynomial_sweep(t, coefs, opts \\ []) do
    opts = Keyword.validate!(opts, phi: 0, phi_unit: :radians)
    coefs = Nx.to_tensor(coefs)

    degrees =
      case opts[:phi_unit] do
        :radians -> 0
        :degrees -> 1
        other -> raise ArgumentError, "polynomial_sweep: phi_unit must be :radians or :degrees, got: #{inspect(other)}"
      end

    if Nx.rank(coefs) != 1 or Nx.size(coefs) < 1 or Nx.size(coefs) > 32 do
      raise ArgumentError, "polynomial_sweep: coefs must be a rank-1 tensor of 1 to 32 entries, got shape #{inspect(Nx.shape(coefs))}"
    end

    {bin, f64, type, shape} = input!(t, "polynomial_sweep")

    if tuple_size(shape) != 1 do
      raise ArgumentError, "polynomial_sweep: t must have rank 1, got shape #{inspect(shape)}"
    end

    cb = coefs |> Nx.as_type({:f, 64}) |> Nx.to_binary()
    {:ok, out} = NIF.polynomial_sweep(NxSignalAMD.context(), bin, f64, cb, opts[:phi], degrees) |> NxSignalAMD.unwrap!()
    tensor(out, type, shape)
  end

  @doc """
  See `NxSignal.Waveforms.unit_impulse/2`. Options `:index` (a number, a tensor of `rank` entries or `:midpoint`; default 0) and
  `:type` (default `:f32`).
  """
  def unit_impulse(shape, opts \\ []) when is_tuple(shape) do
    opts = Keyword.validate!(opts, index: 0, type: :f32)
    type = Nx.Type.normalize!(opts[:type])
    dims = Tuple.to_list(shape)
    rank = length(dims)

    dtype =
      case Map.fetch(@dtypes, type) do
        {:ok, code} -> code
        :error -> raise ArgumentError, "unit_impulse: type must be one of f32, f64, s32, s64, u32, u64, got: #{inspect(type)}"
      end

    if rank > 8 do
      raise ArgumentError, "unit_impulse: rank must be at most 8, got #{rank}"
    end

    index =
      case opts[:index] do
        :midpoint -> Enum.map(dims, &div(&1, 2))
        index -> index |> Nx.to_tensor() |> Nx.reshape({rank}) |> Nx.to_flat_list()
      end

    if 0 not in dims do
      for {i, n, d} <- Enum.zip([index, dims, 0..(rank - 1)//1]), not is_integer(i) or i < 0 or i >= n do
        raise ArgumentError, "unit_impulse: index #{inspect(i)} is out of range for axis #{d} of size #{n}"
      end
    end

    {:ok, out} = NIF.unit_impulse(NxSignalAMD.context(), dtype, dims, index) |> NxSignalAMD.unwrap!()
    tensor(out, type, shape)
  end

  # {binary, is_f64, type, shape} of a real tensor: f64 stays, everything else is read as f32
  defp input!(t, fun) do
    t = Nx.to_tensor(t)

    case Nx.type(t) do
      {:c, _} -> raise ArgumentError, "#{fun}: complex tensors are not supported"
      {:f, 64} -> {Nx.to_binary(t), 1, {:f, 64}, Nx.shape(t)}
      _ -> {t |> Nx.as_type({:f, 32}) |> Nx.to_binary(), 0, {:f, 32}, Nx.shape(t)}
    end
  end

  defp tensor(bin, type, shape), do: bin |> Nx.from_binary(type) |> Nx.reshape(shape)
end
