defmodule NxSignalAMD.PeakFinding do
  @moduledoc """
  `NxSignal.PeakFinding.argrelmin/2`, `argrelmax/2` and `argrelextrema/3` (lib/nx_signal/peak_finding.ex) for host tensors, on the
  GPU kernels of DESIGN.md section 3.9.  Each returns `%{indices: s32 {size, rank}, valid_indices: u32 scalar}`: the coordinates of
  the marked elements in row-major order, then `-1` rows.

  Options: `:axis` (default 0, negative counts from the end) and `:order` (default 1; an order of 0 or less marks every element).
  `Nx.less/2`, `greater/2`, `less_equal/2` and `greater_equal/2` (as captures or atoms) run fused in one kernel; any other
  comparator builds the mask with Nx and only its compaction runs on the GPU.
  """
  alias NxSignalAMD.NIF

  @comparators %{less: 0, greater: 1, less_equal: 2, greater_equal: 3}

  def argrelmin(data, opts \\ []), do: argrelextrema(data, :less, opts)

  def argrelmax(data, opts \\ []), do: argrelextrema(data, :greater, opts)

  def argrelextrema(data, comparator, opts \\ []) do
    opts = Keyword.validate!(opts, axis: 0, order: 1)
    data = Nx.to_tensor(data)
    {axis, shifts} = check!(data, opts[:axis], opts[:order])

    case fused(comparator) do
      nil -> custom(data, comparator, axis, shifts)
      code -> fused_call(data, code, axis, shifts)
    end
  end

  defp check!(data, axis, order) do
    rank = Nx.rank(data)
    shape = Tuple.to_list(Nx.shape(data))

    cond do
      rank == 0 -> raise ArgumentError, "argrelextrema: a rank-0 tensor has no axis"
      rank > 8 -> raise ArgumentError, "argrelextrema: rank must be at most 8, got #{rank}"
      not is_integer(axis) or axis < -rank or axis >= rank -> raise ArgumentError, "argrelextrema: axis #{inspect(axis)} is out of range for rank #{rank}"
      not is_number(order) -> raise ArgumentError, "argrelextrema: order must be a number, got: #{inspect(order)}"
      match?({:c, _}, Nx.type(data)) -> raise ArgumentError, "argrelextrema: complex tensors have no order"
      Enum.any?(shape, &(&1 < 1)) -> raise ArgumentError, "argrelextrema: empty dimension in shape #{inspect(Nx.shape(data))}"
      Enum.any?(shape, &(&1 >= 2_147_483_648)) -> raise ArgumentError, "argrelextrema: every dimension must be below 2^31"
      Nx.size(data) >= 4_294_967_296 -> raise ArgumentError, "argrelextrema: the tensor must have fewer than 2^32 elements"
      true -> {rem(axis + rank, rank), shifts(order)}
    end
  end

  # the shifts s = 1, 2, ... with s < order + 1
  defp shifts(order) when order <= 0, do: 0
  defp shifts(order) when is_integer(order), do: order
  defp shifts(order), do: order |> Float.ceil() |> trunc()

  defp fused(name) when is_atom(name), do: Map.get(@comparators, name)

  defp fused(fun) when is_function(fun, 2) do
    info = Function.info(fun)

    if info[:type] == :external and info[:module] == Nx do
      Map.get(@comparators, info[:name])
    end
  end

  defp fused(_), do: nil

  # widened exactly to a kernel type: f32, f64, s32, s64, u32, u64
  defp kernel_type({:f, 64}), do: {{:f, 64}, 1}
  defp kernel_type({:f, _}), do: {{:f, 32}, 0}
  defp kernel_type({:bf, _}), do: {{:f, 32}, 0}
  defp kernel_type({:s, 64}), do: {{:s, 64}, 3}
  defp kernel_type({:u, 64}), do: {{:u, 64}, 5}
  defp kernel_type({:u, 32}), do: {{:u, 32}, 4}
  defp kernel_type(_), do: {{:s, 32}, 2}

  defp fused_call(data, code, axis, shifts) do
    {type, dtype} = kernel_type(Nx.type(data))
    xb = data |> Nx.as_type(type) |> Nx.to_binary()
    shape = Tuple.to_list(Nx.shape(data))

    {:ok, indices, valid} =
      NIF.argrelextrema(NxSignalAMD.context(), xb, dtype, shape, axis, shifts, code) |> NxSignalAMD.unwrap!()

    result(indices, valid, data)
  end

  defp custom(data, comparator, axis, shifts) when is_function(comparator, 2) do
    n = Nx.axis_size(data, axis)
    locs = Nx.iota({n})
    mask = Nx.broadcast(Nx.u8(1), Nx.shape(data))

    mask =
      Enum.reduce_while(1..max(min(shifts, max(n - 1, 1)), 1)//1, mask, fn s, acc ->
        if s > shifts do
          {:halt, acc}
        else
          plus = Nx.take(data, Nx.clip(Nx.add(locs, s), 0, n - 1), axis: axis)
          minus = Nx.take(data, Nx.clip(Nx.subtract(locs, s), 0, n - 1), axis: axis)
          acc = acc |> Nx.logical_and(comparator.(data, plus)) |> Nx.logical_and(comparator.(data, minus))
          if Nx.to_number(Nx.any(acc)) == 1, do: {:cont, acc}, else: {:halt, acc}
        end
      end)

    mb = mask |> Nx.as_type({:u, 8}) |> Nx.to_binary()
    {:ok, indices, valid} = NIF.nonzero(NxSignalAMD.context(), mb, Tuple.to_list(Nx.shape(data))) |> NxSignalAMD.unwrap!()
    result(indices, valid, data)
  end

  defp custom(_data, comparator, _axis, _shifts) do
    raise ArgumentError, "argrelextrema: the comparator must be a function of arity 2 or one of #{inspect(Map.keys(@comparators))}, got: #{inspect(comparator)}"
  end

  defp result(indices, valid, data) do
    %{
      indices: indices |> Nx.from_binary({:s, 32}) |> Nx.reshape({Nx.size(data), Nx.rank(data)}),
      valid_indices: Nx.tensor(valid, type: {:u, 32})
    }
  end
end
