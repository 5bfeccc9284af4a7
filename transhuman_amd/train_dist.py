"""Data-parallel training: one process per GPU, the gradients averaged by ONE collective per step.

The reference wraps its network in SyncBatchNorm + DistributedDataParallel(find_unused_parameters=True)
(lib/train/trainers/trainer.py:23-33) and deals the data set with its own DistributedSampler (lib/datasets/samplers.py:73-133,
make_dataset.py:77-78).  DDP's buckets, hooks and unused-parameter search are built for overlap with a backward that is long
against the exchange; here the whole gradient is 28 MB behind a ~59 ms step, so the exchange is three steps in a row:

    pack        one launch (csrc/k_optim.hip, adam_pack_kernel) writes g_i / world of every tensor that has a gradient on
                SOME rank into its slot of one flat buffer -- zeros where this rank has none, zeros in the padding
    all-reduce  one SUM over that buffer (RCCL; gloo for host tensors and for the one-GPU multi-rank check)
    views       p.grad of every such tensor becomes a view of its slot, and DeviceAdam steps straight out of the buffer

Which tensors have a slot is agreed on through a host bitmap ("p.grad is not None", known without asking the device) that is
all-reduced (MAX) over a gloo group of the exchange's own, so every rank uses the same layout -- and the same collective size
-- in the same step.  A tensor no rank has a gradient for keeps ``grad = None``: the optimiser skips it and gives it no state,
which is what find_unused_parameters=True amounts to.  With DeviceAdam(zero_grad=True) the zeroed views stay in place, the next
backward accumulates into the buffer and pack divides in place.

The layout rule (``flat_layout``; th_adam_flat_layout is the same rule in C): slots follow the order of the parameter list
and exist only for live tensors, each slot starts at a multiple of 4 elements, and the buffer ends at the last slot's end
rounded up to 4.

The sum of an all-reduce is taken in the collective's order, not in rank order; with two ranks that is one addition and has
no order.  ``grad_exchange_oracle`` is the rank-ordered statement the tests hold the exchange against: bit for bit with two
ranks; with three, one all_reduce cannot meet 2 * 2^-24 * sum_r |g_r / 3| against it (two orders of one three-term sum are each
two roundings from the exact sum: up to 4 * 2^-24 * sum apart; measured over gloo, 0.47 % of 7.4 M elements beyond the former,
none beyond the latter).  ``reduce="ordered"`` is the form that does meet it, at world times the traffic, on request only.

``reduce="rank_ordered"`` meets it at the traffic of a ring all-reduce: a reduce-scatter whose additions this project owns,
then an all-gather.  With slice = ceil(flat_elems / world / 4) * 4 (``rank_slice``) the buffer is world slices long (its tail
past flat_elems is zero and stays zero), and a step is

    pack        as above
    scatter     all_to_all_single with equal splits: rank r receives slice r of every rank's buffer, parts [world, slice]
    sum         one launch (csrc/k_optim.hip, rank_sum_kernel, K28): ((parts[0] + parts[1]) + parts[2]) + ... in fp32, in rank
                order -- the oracle's sum, for any world
    gather      all_gather_into_tensor of the summed slices back into the flat buffer
    views       as above

A rank receives 2 * (world - 1) * slice * 4 bytes (``GradExchange.bytes_received`` counts them), "ordered"
(world - 1) * flat_elems * 4.
"""
import math

import numpy as np
import torch


# ---------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------
def flat_layout(counts, live=None):
    """-> (offsets, flat_elems): the first element of each tensor's slot (-1: no slot) and the length of the flat buffer.
    A pure function of the element counts and the bitmap."""
    offsets, end = [], 0
    for i, n in enumerate(counts):
        n = int(n)
        if n < 1:
            raise ValueError(f"flat_layout: tensor {i} has no elements")
        if live is None or live[i]:
            offsets.append(end)
            end = (end + n + 3) // 4 * 4
        else:
            offsets.append(-1)
    return np.array(offsets, dtype=np.int64), end


def rank_slice(flat_elems, world):
    """elements per rank of the rank-ordered exchange: the flat buffer cut into ``world`` equal slices of whole float4 groups"""
    return (int(flat_elems) + 4 * int(world) - 1) // (4 * int(world)) * 4


def grad_exchange_oracle(per_rank_grads, world):
    """per_rank_grads[r][i]: the gradient of tensor i on rank r (an array, or None) -> per tensor the average the exchange
    defines -- every rank's gradient divided by ``world`` in fp32 (one rounding; a rank without one contributes zeros), the
    ranks added in rank order -- or None where no rank has a gradient."""
    world = int(world)
    if len(per_rank_grads) != world:
        raise ValueError(f"grad_exchange_oracle: {len(per_rank_grads)} gradient lists for {world} ranks")
    w = np.float32(world)
    out = []
    with np.errstate(all="ignore"):
        for gs in zip(*per_rank_grads):
            have = [g for g in gs if g is not None]
            if not have:
                out.append(None)
                continue
            shape = np.asarray(have[0]).shape
            acc = None
            for g in gs:
                term = np.zeros(shape, np.float32) if g is None else np.asarray(g, dtype=np.float32)
                if world != 1:
                    term = term / w
                acc = term if acc is None else acc + term
            assert acc.dtype == np.float32
            out.append(acc)
    return out


# ---------------------------------------------------------------------------
# the data set, dealt to the ranks
# ---------------------------------------------------------------------------
class DistributedSampler(torch.utils.data.Sampler):
    """samplers.py:73-133: the permutation of epoch ``e`` is torch.randperm under manual_seed(e) (shuffle) or the identity,
    padded by wrapping around to num_replicas * ceil(n / num_replicas) indices; rank r takes the r-th contiguous block.
    ``n`` is the data set's length or the data set itself."""

    def __init__(self, n, num_replicas=None, rank=None, shuffle=True):
        if num_replicas is None or rank is None:
            import torch.distributed as dist
            num_replicas = dist.get_world_size() if num_replicas is None else num_replicas
            rank = dist.get_rank() if rank is None else rank
        self.n = int(n) if isinstance(n, (int, np.integer)) else len(n)
        self.num_replicas, self.rank = int(num_replicas), int(rank)
        if not 0 <= self.rank < self.num_replicas:
            raise ValueError(f"DistributedSampler: rank {rank} of {num_replicas}")
        self.epoch = 0
        self.num_samples = int(math.ceil(self.n * 1.0 / self.num_replicas))
        self.total_size = self.num_samples * self.num_replicas
        self.shuffle = shuffle

    def __iter__(self):
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.epoch)
            indices = torch.randperm(self.n, generator=g).tolist()
        else:
            indices = list(range(self.n))
        indices += indices[: (self.total_size - len(indices))]
        assert len(indices) == self.total_size
        offset = self.num_samples * self.rank
        return iter(indices[offset:offset + self.num_samples])

    def __len__(self):
        return self.num_samples

    def set_epoch(self, epoch):
        self.epoch = epoch


def iterations_per_rank(max_iter, world):
    """make_dataset.py:77-78: an epoch of cfg.ep_iter iterations is shared out, each rank runs int(max_iter / world)"""
    return int(max_iter / world)


# ---------------------------------------------------------------------------
# the exchange
# ---------------------------------------------------------------------------
def _dist():
    import torch.distributed as dist
    return dist if dist.is_available() and dist.is_initialized() else None


class _Layout:
    """the flat buffer of one bitmap: offsets, the buffer, a view of it per live tensor in the tensor's shape"""

    def __init__(self, params, counts, live, slices=1):
        self.offsets, self.flat_elems = flat_layout(counts, live)
        self.live = [i for i, l in enumerate(live) if l]
        ref = params[0]
        # (slices > 1, the rank-ordered exchange: `slices` whole slices; pack never writes the tail, which stays zero)
        self.slice = rank_slice(self.flat_elems, slices)
        self.flat = torch.zeros(max(self.flat_elems, 4, slices * self.slice), dtype=torch.float32, device=ref.device)
        self.parts = None                # (rank-ordered exchange) what the scatter delivers, [slices * slice]
        self.views, self.pads = {}, []
        for i in self.live:
            o, n = int(self.offsets[i]), counts[i]
            self.views[i] = self.flat[o:o + n].view(params[i].shape)
            if n % 4:
                self.pads.append((o + n, (o + n + 3) // 4 * 4))
        self.view_ptrs = None            # (device back end) the addresses of a step whose gradients all ARE the views


class GradExchange:
    """Averages the gradients of ``params`` over the ranks of ``group`` with one collective per step (module docstring).

    group: the process group of the all-reduce (None: the default group, when torch.distributed is initialised; without a
    process group the exchange is local -- pack and views only -- and ``world`` defaults to 1).  ``world`` / ``rank`` override
    what the group says (a local exchange may divide by any ``world``).  Construction is a collective when there is a group:
    every rank builds its exchange at the same point (it opens a gloo group for the bitmap).

    Two back ends with the same results: parameters on a device go through adam_pack_kernel (HipError for anything but
    contiguous fp32 tensors: nothing is converted silently), host parameters through torch (``div`` into the slot) -- what the
    host tests run over gloo and what the device is held against.  ``backend="torch"`` forces the second one.

    reduce: "collective" (the default, on every transport) is the ONE all_reduce(SUM) of the flat buffer.  The order of its
    additions is the collective's: two ranks equal the rank-ordered oracle bit for bit, three and more give the fp32 sum in
    SOME order, which can differ from the oracle by up to 4 * 2^-24 * sum_r |g_r / world| with three ranks (gloo's ring
    starts every chunk at another rank).  "ordered", only ever on request, gathers the ranks' buffers (all_gather: world times
    the traffic) and adds them in rank order, which IS the oracle, bit for bit, for any world: a yardstick, not a way to train.
    "rank_ordered" is the oracle bit for bit as well, at a ring all-reduce's traffic (module docstring): all_to_all_single, the
    rank-ordered sum of the received slices (th_rank_sum on the device back end, torch additions on the host one),
    all_gather_into_tensor.  Over RCCL the device buffers are the collectives' own operands; over gloo, which is only the test
    transport, device buffers are staged through host memory.  ``bytes_received`` counts what the gathers and scatters of
    "ordered" and "rank_ordered" delivered to this rank from the others (the all_reduce's share is the collective's business).

    Liveness with DeviceAdam(zero_grad=True): a zeroed view stays ``p.grad``, so "has a gradient" stays true for a tensor
    that once had a slot, and the bitmap only grows.  A branch that stops taking part keeps its slot and is stepped on zero
    gradients (its moments decay, it still moves) -- unlike find_unused_parameters=True, which skips it.  An optimiser whose
    zero_grad() sets the gradients to None (DeviceAdam's default, torch's default) gives the bitmap of each step on its own.

    ``group`` other than the default one: the bitmap's gloo group is made of the same ranks; torch.distributed.new_group is a
    collective of the WHOLE job, so every process of the job, member or not, has to construct its exchange at the same point.

    Every layout keeps its flat buffer (the layouts of a run are few: the bitmap changes only when a branch of the network
    starts or stops taking part)."""

    def __init__(self, params, group=None, world=None, rank=None, backend=None, reduce=None):
        self.params = [p for p in params]
        if not self.params:
            raise ValueError("GradExchange: no parameters")
        dist = _dist()
        self.dist = dist
        self.group = group
        self.world = int(world) if world is not None else (dist.get_world_size(group) if dist else 1)
        self.rank = int(rank) if rank is not None else (dist.get_rank(group) if dist else 0)
        if self.world < 1:
            raise ValueError(f"GradExchange: world = {self.world}")
        # the bitmap's own communicator: host memory, never queued behind the gradient's collective (dist.DeferredSum)
        self.host_group = dist.new_group(ranks=None if group is None else dist.get_process_group_ranks(group),
                                         backend="gloo") if dist else None
        first = self.params[0]
        if backend not in (None, "device", "torch"):
            raise ValueError(f"GradExchange: backend = {backend!r}")
        self.backend = backend or ("device" if first.is_cuda else "torch")
        if reduce not in (None, "collective", "ordered", "rank_ordered"):
            raise ValueError(f"GradExchange: reduce = {reduce!r}")
        self.reduce = reduce or "collective"
        for i, p in enumerate(self.params):
            if p.device != first.device or p.dtype is not torch.float32 or p.numel() == 0:
                raise ValueError(f"GradExchange: parameter {i} is {p.dtype} on {p.device} with {p.numel()} elements; "
                                 f"fp32 tensors on {first.device} are exchanged")
        self.counts = [p.numel() for p in self.params]
        self._layouts = {}
        self._plan = None
        self._world_t = torch.tensor(float(self.world), dtype=torch.float32, device=first.device)
        self.layout = None               # the layout of the last exchange
        self.exchanges = 0
        self.bytes_received = 0

    # -- layouts -----------------------------------------------------------------------------------------------------
    def _bitmap(self):
        live = np.fromiter((p.grad is not None for p in self.params), dtype=np.uint8, count=len(self.params))
        if self.dist is not None:
            t = torch.from_numpy(live)
            self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX, group=self.host_group)
        return live

    def _layout_of(self, live):
        key = live.tobytes()
        lay = self._layouts.get(key)
        if lay is None:
            slices = self.world if self.reduce == "rank_ordered" and self.dist is not None else 1
            lay = self._layouts[key] = _Layout(self.params, self.counts, live, slices)
        return lay

    # -- pack --------------------------------------------------------------------------------------------------------
    def _pack_device(self, lay, grads):
        from . import hip
        if self._plan is None:
            self._plan = hip.AdamPlan(self.params)
        if lay.view_ptrs is not None and all(grads[i] is lay.views[i] for i in lay.live):
            self._plan.pack(lay.view_ptrs, lay.offsets, self.world, lay.flat, lay.flat_elems)     # the steady state
            return
        ptrs = self._plan.pack(grads, lay.offsets, self.world, lay.flat, lay.flat_elems)
        if all(grads[i] is lay.views[i] for i in lay.live):
            lay.view_ptrs = ptrs

    def _pack_torch(self, lay, grads):
        for i in lay.live:
            slot, g = lay.views[i], grads[i]
            if g is None:
                slot.zero_()
            elif self.world == 1:
                if g is not slot:
                    slot.copy_(g)
            else:
                torch.div(g, self._world_t, out=slot)          # (a tensor divisor: a true division, not a reciprocal's product)
        for a, b in lay.pads:
            lay.flat[a:b] = 0

    # -- the rank-ordered reduce-scatter + all-gather ------------------------------------------------------------------
    def _rank_ordered(self, lay):
        dist, world, n = self.dist, self.world, lay.slice
        full = lay.flat[:world * n]
        if lay.parts is None:
            lay.parts = torch.empty_like(full)
        parts = lay.parts
        # the sum lands on one of the parts: the rank's own on the device, rank 0's (only ever the first term) on the host
        mine = parts[self.rank * n:(self.rank + 1) * n] if self.backend == "device" else parts[:n]
        staged = full.is_cuda and dist.get_backend(self.group) == "gloo"
        if staged:
            host = torch.empty(world * n, dtype=torch.float32)
            dist.all_to_all_single(host, full.cpu(), group=self.group)
            parts.copy_(host)
        else:
            dist.all_to_all_single(parts, full, group=self.group)
        if self.backend == "device":
            from . import hip
            hip.rank_sum(parts, world, n, mine)
        else:
            for r in range(1, world):                          # one fp32 addition per rank, in rank order
                mine.add_(parts[r * n:(r + 1) * n])
        if staged:
            dist.all_gather_into_tensor(host, mine.cpu(), group=self.group)
            full.copy_(host)
        else:
            dist.all_gather_into_tensor(full, mine, group=self.group)
        self.bytes_received += 2 * (world - 1) * n * 4

    # -- the step ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def exchange(self):
        """after loss.backward(): averages the gradients over the ranks; afterwards ``p.grad`` of every tensor that has a
        gradient on some rank is a view of the flat buffer, on every rank.  Returns the flat buffer's live part."""
        live = self._bitmap()
        lay = self.layout = self._layout_of(live)
        self.exchanges += 1
        if lay.flat_elems == 0:
            return lay.flat[:0]
        grads = [None] * len(self.params)
        for i in lay.live:
            g = self.params[i].grad
            if g is not None:
                if g.is_sparse:
                    raise RuntimeError("GradExchange does not exchange sparse gradients")
                if g.dtype is not torch.float32 or g.device != lay.flat.device:
                    raise ValueError(f"GradExchange: the gradient of parameter {i} is {g.dtype} on {g.device}")
                if not g.is_contiguous():
                    g = g.contiguous()
            grads[i] = g
        flat = lay.flat[:lay.flat_elems]
        (self._pack_device if self.backend == "device" else self._pack_torch)(lay, grads)
        if self.dist is not None:
            if self.reduce == "ordered" and self.world > 1:
                parts = [torch.empty_like(flat) for _ in range(self.world)]
                self.dist.all_gather(parts, flat, group=self.group)
                flat.copy_(parts[0])
                for part in parts[1:]:
                    flat.add_(part)                            # one fp32 addition per rank, in rank order
                self.bytes_received += (self.world - 1) * lay.flat_elems * 4
            elif self.reduce == "rank_ordered" and self.world > 1:
                self._rank_ordered(lay)
            else:
                self.dist.all_reduce(flat, op=self.dist.ReduceOp.SUM, group=self.group)
        for i in lay.live:
            p = self.params[i]
            if p.grad is not lay.views[i]:
                p.grad = lay.views[i]
        if self.backend == "device":
            # pack wrote through raw pointers: a gradient that was its own slot changed without autograd's knowledge
            torch.autograd.graph.increment_version(lay.flat)     # (its views share the counter)
        return flat

    # -- the start ---------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def broadcast_parameters(self, module, src=0):
        """every rank takes the parameters and buffers of rank ``src`` (a global rank): the fp32 tensors travel as ONE
        buffer (pack at world = 1, broadcast, unpack), the few others (BatchNorm's num_batches_tracked) one by one"""
        if self.dist is None:
            return
        tensors = [p.detach() for p in module.parameters()] + [b for b in module.buffers()]    # (detach: p's own version counter)
        dev = self.params[0].device
        flat_ok = [t for t in tensors if t.dtype is torch.float32 and t.is_contiguous() and t.numel() > 0 and t.device == dev]
        taken = {id(t) for t in flat_ok}
        rest = [t for t in tensors if id(t) not in taken and t.numel() > 0]
        if flat_ok:
            counts = [t.numel() for t in flat_ok]
            offsets, n = flat_layout(counts)
            flat = torch.zeros(n, dtype=torch.float32, device=dev)
            if self.backend == "device":
                from . import hip
                plan = hip.AdamPlan(flat_ok)
                plan.pack(flat_ok, offsets, 1, flat, n)
                self.dist.broadcast(flat, src=src, group=self.group)
                plan.unpack(flat_ok, offsets, flat, n)
                torch.cuda.current_stream(dev).synchronize()   # (the plan and the buffer go out of scope here)
                torch.autograd.graph.increment_version(flat_ok)
            else:
                for t, o in zip(flat_ok, offsets):
                    flat[int(o):int(o) + t.numel()] = t.reshape(-1)
                self.dist.broadcast(flat, src=src, group=self.group)
                for t, o in zip(flat_ok, offsets):
                    t.copy_(flat[int(o):int(o) + t.numel()].view(t.shape))
        for t in rest:
            self.dist.broadcast(t, src=src, group=self.group)
