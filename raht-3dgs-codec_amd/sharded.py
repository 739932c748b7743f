"""Morton-prefix sharded RAHT (BASELINE.json configs[4]).

A large scene is partitioned across the GPUs of one node by contiguous ranges of the top
``prefix_bits`` (= 9: three octree levels) bits of the Morton key. Every butterfly below those
levels pairs rows that share the prefix, so it is shard-local; each shard is left with one low-pass
row per non-empty prefix node (<= 512 rows in total over all shards). ONE small all-gather of those
rows (<= 512 x D floats ~ 121 KB at D = 59: latency-bound on xGMI) lets every GPU redundantly run
the top 9 binary levels on a weighted <= 512-row tree and keep the coefficients of its own prefixes.
The inverse mirrors it: gather the top coefficients, invert the top tree, continue shard-locally.

What one direction of a step enqueues besides the shard-local transform -- nothing else, no torch ops:

    forward   local kernels write their root rows STRAIGHT into this rank's slot of the send buffer
              -> all_gather_into_tensor (padded slots of max_roots rows per rank)
              -> ONE launch of the replicated top tree, in place on the padded gather buffer (row map)
              -> ONE launch that quantizes this rank's top coefficients into their places in Q
                 (or scatters them into T)
    inverse   ONE launch dequantizes (gathers) this rank's top coefficients into the send buffer
              -> all_gather_into_tensor -> ONE launch of the top tree
              -> local kernels read their roots straight from this rank's slot of the result

A quantized step runs over LANES: one (the quantizer's float type, all D columns) for n_wide = 0; two for n_wide > 0, the
float lane on columns [n_wide, D) and the wide (float64) lane on columns [0, n_wide), each with a buffer set of its own.
Whatever is per lane above happens float lane first: both gathers, then both top trees, then both row quantizer launches.

One process per GPU, ``torch.distributed`` (backend "nccl" = RCCL on ROCm; gloo in the CPU tests).
The shard-local work goes through the C ABI (``ops.RahtPlan``); ``local_ops`` lets the CPU tests
inject a reference implementation of the same interface -- the product default has no CPU path.

Un-partitioned input (every rank holds an arbitrary part of the cloud): ``exchange_by_prefix`` is the
distributed counterpart of the reference's single ``torch.sort`` (python/voxelize_pc.py:97-118): global
bounding box, 512-bin prefix histogram, balanced cuts, ONE all-to-all of the points by destination rank,
then the local voxelizer (stable radix sort + per-voxel mean) on what arrived.
"""
import collections

import torch

from . import _lib, ops


def _dist():
    import torch.distributed as dist
    return dist if dist.is_available() and dist.is_initialized() else None


class _Collectives:
    """The process group as this module uses it: who we are in it, and whether CUDA tensors have to be staged through the
    host (the test / debugging configuration: several ranks sharing one GPU over a CPU-only backend). With no process
    group: a world of one, and no method below may be called."""

    def __init__(self, group=None):
        self.dist, self.group = _dist(), group
        self.world = self.dist.get_world_size(group) if self.dist else 1
        self.rank = self.dist.get_rank(group) if self.dist else 0
        self.host_staged = bool(self.dist) and self.dist.get_backend(group) == "gloo"

    def all_gather(self, x, out=None):
        """all-gather a (rows, cols) tensor -> (world * rows, cols)."""
        if self.host_staged and x.is_cuda:
            got = self.all_gather(x.contiguous().cpu())
            return got.to(x.device) if out is None else out.copy_(got)
        if out is None:
            out = torch.empty((self.world * x.shape[0], x.shape[1]), dtype=x.dtype, device=x.device)
        self.dist.all_gather_into_tensor(out, x, group=self.group)
        return out

    def _host(self, t):
        return t.cpu() if self.host_staged and t.is_cuda else t

    def all_reduce(self, t, op):
        """-> t reduced over the ranks by ReduceOp.<op> ("MIN", "MAX", "SUM"); in place unless staged"""
        c = self._host(t)
        self.dist.all_reduce(c, op=getattr(self.dist.ReduceOp, op), group=self.group)
        return c.to(t.device)

    def all_to_all_rows(self, send, counts):
        """send: rows grouped by destination rank, counts[r] of them for rank r. -> (the rows that arrived, in source rank
        order; rows sent to every rank; rows received from every rank)"""
        dev, send, counts = send.device, self._host(send), self._host(counts)
        arrived = torch.empty_like(counts)
        self.dist.all_to_all_single(arrived, counts, group=self.group)
        ss, rs = counts.tolist(), arrived.tolist()
        recv = torch.empty((sum(rs), send.shape[1]), dtype=send.dtype, device=send.device)
        self.dist.all_to_all_single(recv, send, output_split_sizes=rs, input_split_sizes=ss, group=self.group)
        return recv.to(dev), ss, rs

    def barrier(self):
        self.dist.barrier(group=self.group)


def cuts_from_histogram(hist, world):
    """Prefix boundaries [0 = c_0 <= c_1 <= ... <= c_world = len(hist)] that balance the row counts of
    ``world`` contiguous prefix ranges: rank r owns prefixes [c_r, c_{r+1})."""
    cum = torch.cumsum(hist.to(torch.int64), 0).cpu().tolist()                    # rows with prefix <= p
    nb = len(cum)
    N = cum[-1] if cum else 0
    cuts, lo = [0], 0
    for r in range(1, world):
        target = N * r / world
        # the prefix boundary whose row count is closest to the target, never moving backwards
        best, best_err = lo, None
        for p in range(lo, nb + 1):
            rows_below = cum[p - 1] if p > 0 else 0
            err = abs(rows_below - target)
            if best_err is None or err < best_err:
                best, best_err = p, err
            if rows_below > target:
                break
        lo = best
        cuts.append(best)
    cuts.append(nb)
    return cuts


def balanced_prefix_cuts(keys_sorted, nbits, world, prefix_bits=9):
    """Where to cut a Morton-sorted scene into `world` shards: row boundaries
    [0 = b_0 <= b_1 <= ... <= b_world = N] such that every cut falls between two different values of
    the top ``prefix_bits`` key bits, balanced by the 2^prefix_bits-bin population histogram. Shard r =
    rows [b_r, b_{r+1}); hand each to one rank's ``ShardedRaht``. Works on CPU or GPU tensors."""
    N = int(keys_sorted.shape[0])
    nb = 1 << prefix_bits
    pref = (keys_sorted.to(torch.int64) >> (nbits - prefix_bits)).clamp_(0, nb - 1)
    hist = torch.bincount(pref, minlength=nb)
    pc = cuts_from_histogram(hist, world)
    cum = [0] + torch.cumsum(hist, 0).cpu().tolist()
    out = [cum[p] for p in pc]
    out[-1] = N
    return out


class HipLocalOps:
    """Shard-local operations on the MI355X through libraht_hip.so."""
    quant_dtype = torch.float32          # arithmetic type of the fused quantize / dequantize kernels

    @staticmethod
    def make_plan(keys, nbits, top_level=None, leaf_weights=None):
        return ops.RahtPlan.from_keys(keys, nbits, leaf_weights=leaf_weights, top_level=top_level)

    # the few top coefficients, quantized into / dequantized out of their places in Q: one launch each
    quant_rows = staticmethod(ops.quant_rows)
    dequant_rows = staticmethod(ops.dequant_rows)
    # mixed precision (n_wide > 0): the same at float64 for the wide columns of the top coefficients ...
    quant_rows_f64 = staticmethod(ops.quant_rows_f64)
    dequant_rows_f64 = staticmethod(ops.dequant_rows_f64)
    # ... and the shard-local fused passes with the wide columns in float64, roots through the two root buffers: plan methods
    forward_quant_mixed = staticmethod(ops.RahtPlan.forward_quant_mixed)
    dequant_inverse_mixed = staticmethod(ops.RahtPlan.dequant_inverse_mixed)
    rows_gather = staticmethod(ops.rows_gather)
    rows_scatter = staticmethod(ops.rows_scatter)
    # front end (exchange_by_prefix)
    voxel_keys = staticmethod(ops.voxel_keys)
    sort_keys = staticmethod(ops.sort_keys)

    @staticmethod
    def voxelize(PC, vmin, width, J):
        PCvox, _, vidx, _, info = ops.voxelize_pc_batched(PC, vmin, width, J, device=PC.device, residuals=False, sorted_points=False)
        return PCvox, info["keys_sorted"][vidx], vidx, info


MIXED_OPS = ("forward_quant_mixed", "dequant_inverse_mixed", "quant_rows_f64", "dequant_rows_f64")


class _DeviceArray:
    """a raw device pointer as something torch.as_tensor can wrap without copying (__cuda_array_interface__)"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


class _DirectExchange:
    """One direct exchange block (include/raht.h, raht_xchg_*; all of this module's ctypes): this rank's fine-grained device
    block with the two parity gather buffers and their flags, and the peers' blocks mapped over hipIpc. Every rank writes its
    send slot into each peer's block and raises a flag, one launch per gather. Opening is COLLECTIVE; so is closing, in two
    steps with a barrier of the caller's between them: close_peers on every rank, then free."""

    def __init__(self, coll, send, gather_rows):
        """COLLECTIVE: allocate the block for slots the size of ``send``, swap the hipIpc handles through the process group,
        map the peers' blocks, wrap the two gather buffers as (gather_rows, D) tensors."""
        import ctypes as C
        L = _lib.lib()
        self.world, self.rank, self.device = coll.world, coll.rank, send.device
        self.slot_bytes = int(send.numel() * send.element_size())
        self.seq = 0                                            # gathers so far: the flag value and, its low bit, the parity
        self.base, handle = C.c_void_p(), (C.c_ubyte * 64)()
        with torch.cuda.device(self.device):
            _lib.check(L.raht_xchg_alloc(self.world, self.slot_bytes, C.byref(self.base), handle))
        handles = [None] * self.world
        coll.dist.all_gather_object(handles, bytes(handle), group=coll.group)
        self.peers = (C.c_void_p * self.world)()
        for r in range(self.world):
            if r == self.rank:
                self.peers[r] = self.base.value
            else:
                hb, pb = (C.c_ubyte * 64).from_buffer_copy(handles[r]), C.c_void_p()
                with torch.cuda.device(self.device):
                    _lib.check(L.raht_xchg_open(hb, C.byref(pb)))
                self.peers[r] = pb.value
        typestr = {torch.float32: "<f4", torch.float64: "<f8"}[send.dtype]
        self.views = []
        for par in (0, 1):
            p = C.c_void_p()
            _lib.check(L.raht_xchg_buffer(self.base, self.world, self.slot_bytes, par, C.byref(p)))
            self.views.append(torch.as_tensor(_DeviceArray(p.value, (gather_rows, send.shape[1]), typestr), device=self.device))
        coll.barrier()                                          # nobody writes into a block that is not mapped yet

    def gather(self, send, stream):
        """ONE launch on ``stream``: write ``send`` into every rank's block, wait (bounded) for theirs. -> the gather buffer
        this round fills; the two alternate."""
        import ctypes as C
        self.seq += 1
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().raht_xchg_gather(C.c_void_p(send.data_ptr()), self.slot_bytes, self.peers, self.rank, self.world,
                                                   self.seq & 0xffffffff, C.c_void_p(stream)))
        return self.views[self.seq & 1]

    def status(self, stream):
        """(synchronises) 0 = every gather so far met all of its peers; 1 = a wait timed out"""
        import ctypes as C
        st = C.c_int()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().raht_xchg_status(self.base, self.world, self.slot_bytes, C.c_void_p(stream), C.byref(st)))
        return st.value

    def close_peers(self):
        for r in range(self.world):
            if r != self.rank:
                _lib.check(_lib.lib().raht_xchg_close(self.peers[r]))

    def free(self):
        """once every rank has unmapped this block"""
        self.views = None
        _lib.check(_lib.lib().raht_xchg_free(self.base))


class _RootBuffers:
    """One buffer set of root rows: send (slot x D: this rank's roots), recv (world * slot x D: everybody's -- the CURRENT
    receive buffer: the direct exchange alternates between two), res (the top tree's output, same layout); send_roots and
    mine are this rank's rows of send and res. With one rank and no collective, recv IS send."""
    __slots__ = ("send", "send_roots", "recv", "res", "mine", "exchange")

    def __init__(self, send, recv, res, lo, n_roots, exchange):
        self.send, self.recv, self.res, self.exchange = send, recv, res, exchange
        self.send_roots, self.mine = send[:n_roots], res[lo: lo + n_roots]

    def gather(self, coll):
        """send -> recv over the ranks: the direct exchange's launch, or the all-gather (none if recv is send)"""
        if self.exchange is not None:
            self.recv = self.exchange.gather(self.send, torch.cuda.current_stream(self.send.device).cuda_stream)
        elif self.recv is not self.send:
            coll.all_gather(self.send, out=self.recv)


# One precision of a quantized step: its buffer set, its columns of Q (None: all of them), the views of the buffer set's
# send_roots and mine that hold those columns, and the row quantizer / dequantizer of its type.
_Lane = collections.namedtuple("_Lane", "bufs cols send_cols mine_cols quant dequant")


class ShardedRaht:
    def __init__(self, keys_sorted, nbits, prefix_bits=9, group=None, local_ops=None, force_collectives=False, direct=False,
                 n_wide=0):
        """keys_sorted: this rank's sorted, unique Morton keys (int64 tensor). Ranks must own disjoint,
        increasing ranges of the top ``prefix_bits`` bits (rank 0 the lowest prefixes).
        force_collectives: issue the all-gathers even in a one-rank group (exercises the RCCL path on one GPU).
        direct: the two all-gathers of a step as DIRECT writes into the peers' gather buffers (_DirectExchange:
        one launch per direction, every rank writes its <= 15 KB slot to each peer over its own xGMI link and raises a flag;
        SURVEY.md 5 / 8e) instead of RCCL's all_gather_into_tensor. Opt-in and EXPERIMENTAL: hipIpc + fine-grained memory +
        peer mapping have only been exercised by ranks sharing ONE GPU (tests/test_gpu_sharded.py); no run over xGMI exists.
        The process group is still used once per (D, dtype) to exchange the hipIpc handles. A peer that never arrives ends a
        bounded wait, not a hung GPU -- and leaves a status word: check_exchange() (called by close(), roundtrip_error(),
        check_against_unsharded()) raises on it, and every later direct gather of the object refuses to run. Call close()
        (collective) before dropping the object.
        n_wide: > 0 (1..4) runs the quantized entries (forward_quant, dequant_inverse, step / local_step with a quantization
        step) in MIXED precision: columns [0, n_wide) -- the xyz columns of a 59-column frame -- in float64 throughout (the
        reference's integers, python/encode_3dgs.py:82-83,204), the others in float32 exactly as with n_wide = 0. The wide
        roots travel in a buffer set of their own ((., n_wide) float64: a second, small gather per direction) and the
        replicated top tree runs once more, in float64, on them. forward / inverse (unquantized) are unchanged."""
        self.ops = local_ops or HipLocalOps
        self.n_wide = int(n_wide)
        if self.n_wide:
            if not 1 <= self.n_wide <= 4:
                raise ValueError("n_wide must be 0 (float32) or 1..4")
            missing = [f for f in MIXED_OPS if not hasattr(self.ops, f)]
            if missing:
                raise ValueError(f"ShardedRaht(n_wide={self.n_wide}): local_ops lacks {', '.join(missing)}")
        self.direct = bool(direct)
        self._direct_failed = False
        self.qdt = getattr(self.ops, "quant_dtype", torch.float32)
        self.coll = _Collectives(group)
        self.world, self.rank = self.coll.world, self.coll.rank
        self._collective = self.world > 1 or (bool(force_collectives) and self.coll.dist is not None)     # do the gathers run at all
        self.nbits, self.prefix_bits = int(nbits), int(prefix_bits)
        if not (0 < self.prefix_bits < self.nbits):
            raise ValueError("prefix_bits must be in (0, nbits)")
        self.N = int(keys_sorted.shape[0])
        dev = keys_sorted.device
        self.device = dev
        self._ev = None                                         # collective timing (time_collectives)
        if self.N > 0:
            # shard-local plan: butterflies at levels >= nbits - prefix_bits are left to the top stage
            self.plan = self.ops.make_plan(keys_sorted, self.nbits, top_level=self.nbits - self.prefix_bits)
            self.root_rows = self.plan.root_rows                # first row of every local prefix node
        else:
            # a rank whose prefix range holds no point (balanced cuts of a very uneven scene, or fewer occupied prefixes
            # than ranks): no local plan, no roots -- but it takes part in every collective like the others
            self.plan = None
            self.root_rows = torch.empty(0, dtype=torch.int64, device=dev)
        self.n_roots = int(self.root_rows.shape[0])
        pref = (keys_sorted[self.root_rows] >> (self.nbits - self.prefix_bits)).to(torch.int64)
        ends = torch.cat([self.root_rows[1:], torch.tensor([self.N], dtype=torch.int64, device=dev)])
        counts = (ends - self.root_rows).to(torch.int64)
        # ---- one-off exchange of the root directory: (prefix id, leaf count) per root, padded slots ----
        sizes = self._all_gather(torch.tensor([[self.n_roots]], dtype=torch.int64, device=dev)).reshape(-1)
        self.sizes = [int(x) for x in sizes.tolist()]
        if max(self.sizes) == 0:
            raise ValueError("ShardedRaht: the scene is empty on every rank")
        self.slot = (max(self.sizes) + 3) // 4 * 4              # rows per rank in the gather buffers (whole 16-byte units per slot)
        self.offset = sum(self.sizes[:self.rank])               # this rank's first entry in the top tree
        directory = torch.zeros((self.slot, 2), dtype=torch.int64, device=dev)
        directory[: self.n_roots, 0] = pref
        directory[: self.n_roots, 1] = counts
        alld = self._all_gather(directory)                      # (world * slot, 2)
        valid = [r * self.slot + i for r in range(self.world) for i in range(self.sizes[r])]
        vidx = torch.tensor(valid, dtype=torch.int64, device=dev)
        allpref, allcnt = alld[vidx, 0].contiguous(), alld[vidx, 1].contiguous()
        if allpref.numel() > 1 and not bool((allpref[1:] > allpref[:-1]).all()):
            raise ValueError("shards must own disjoint, increasing Morton-prefix ranges")
        self.total_rows = int(allcnt.sum().item())
        # ---- the top tree: <= 2^prefix_bits weighted leaves, replicated on every rank, working IN PLACE on the
        # padded gather buffer: entry e of the tree lives in buffer row vidx[e] ----
        self.top = self.ops.make_plan(allpref, self.prefix_bits, leaf_weights=allcnt)
        self.gather_rows = self.world * self.slot
        if self.gather_rows != int(allpref.numel()):          # padded slots: entry e of the tree lives in buffer row vidx[e]
            self.top.set_row_map(vidx, self.gather_rows)
        self._bufs = {}
        self._lane_sets = {}
        self._root_pos = None

    # ---- collectives ------------------------------------------------------------------------------
    def _all_gather(self, x, out=None):
        """all-gather a (rows, cols) tensor -> (world * rows, cols); a group of one gathers only under force_collectives"""
        return self.coll.all_gather(x, out) if self._collective else x

    def _buffers(self, D, dtype):
        """-> the buffer set of (D, dtype), allocated (and, direct=True, its exchange block opened: COLLECTIVE) on first use.
        With one rank the three buffers coincide in size, and unless the gathers are forced no collective runs."""
        key = (int(D), dtype)
        b = self._bufs.get(key)
        if b is None:
            mk = lambda rows: torch.zeros((rows, D), dtype=dtype, device=self.device)    # noqa: E731
            send = mk(self.slot)
            recv = mk(self.gather_rows) if self._collective else send
            xchg = _DirectExchange(self.coll, send, self.gather_rows) if self.direct and self._collective and send.is_cuda else None
            b = self._bufs[key] = _RootBuffers(send, recv, mk(self.gather_rows), self.rank * self.slot, self.n_roots, xchg)
        return b

    def _lanes(self, D):
        """-> (the lanes of a quantized step on D columns, their buffer sets), built once per D"""
        ls = self._lane_sets.get(D)
        if ls is None:
            nw = self.n_wide
            if nw and D - nw < 1:
                raise ValueError(f"ShardedRaht(n_wide={nw}): needs more than n_wide columns")
            b, fl = self._buffers(D, self.qdt), slice(nw, None)
            if not nw:
                lanes = (_Lane(b, None, b.send_roots, b.mine, self.ops.quant_rows, self.ops.dequant_rows),)
            else:
                bw = self._buffers(nw, torch.float64)
                lanes = (_Lane(b, fl, b.send_roots[:, fl], b.mine[:, fl], self.ops.quant_rows, self.ops.dequant_rows),
                         _Lane(bw, slice(0, nw), bw.send_roots, bw.mine, self.ops.quant_rows_f64, self.ops.dequant_rows_f64))
            ls = self._lane_sets[D] = (lanes, tuple(lane.bufs for lane in lanes))
        return ls

    def _lane_steps(self, step, D):
        """-> each lane's step argument: one lane takes ``step`` as it came; two: a scalar stays one, D values split like the columns"""
        if not self.n_wide:
            return (step,)
        st = ops.step_list(step, D)
        if len(st) == 1:
            return st[0], st[0]
        return st[self.n_wide:], st[: self.n_wide]

    def _root_positions(self):
        if self._root_pos is None:
            self._root_pos = self.plan.inv_order[self.root_rows].contiguous() if self.plan is not None else self.root_rows
        return self._root_pos

    # ---- timing of the two collectives of a step (bench.py) ---------------------------------------
    def time_collectives(self, on):
        """on: record an event pair on the current stream around each all-gather of the steps that follow."""
        self._ev = {"fwd": [], "inv": []} if on else None

    def collective_ms(self):
        """-> (forward, inverse) mean milliseconds between the events recorded since time_collectives(True)."""
        torch.cuda.synchronize(self.device)
        out = []
        for k in ("fwd", "inv"):
            ev = self._ev[k]
            out.append(sum(a.elapsed_time(b) for a, b in ev) / max(1, len(ev)))
            ev.clear()
        return tuple(out)

    # ---- direct exchange: status, closing -----------------------------------------------------------
    def _exchanges(self):
        return [b.exchange for b in self._bufs.values() if b.exchange is not None]

    def exchange_status(self):
        """(synchronises) 0 = every direct gather so far met all of its peers; 1 = a wait timed out"""
        worst = 0
        for x in self._exchanges():
            worst = max(worst, x.status(torch.cuda.current_stream(self.device).cuda_stream))
        if worst:
            self._direct_failed = True
        return worst

    def check_exchange(self):
        """(synchronises) Raise if a direct gather timed out: the transforms that followed it ran the top tree on a stale or
        partially written gather buffer and returned without an error (the wait is bounded so that a missing peer cannot
        hang the GPU; what it leaves behind is the status word this reads). Called by close(), roundtrip_error() and
        check_against_unsharded(); a caller of the direct path should call it wherever it synchronises anyway. After a
        timeout every further direct gather of this object raises."""
        if self.exchange_status():
            raise RuntimeError("ShardedRaht(direct=True): a direct gather timed out waiting for a peer (exchange status 1): "
                               "results since then are not valid")

    def close(self):
        """COLLECTIVE: unmap the peers' exchange blocks and free this rank's (direct=True). A block must outlive every peer's
        last write into it, hence the barriers; nothing to do for the RCCL path."""
        xs = self._exchanges()
        if not xs:
            return
        failed = bool(self.exchange_status())                  # (synchronises) reported after the blocks are gone
        torch.cuda.synchronize(self.device)
        self.coll.barrier()
        for x in xs:
            x.close_peers()
        self.coll.barrier()
        self._bufs.clear()                                     # the views of the blocks go with them
        self._lane_sets.clear()
        for x in xs:                                           # the blocks themselves: every rank has unmapped them
            x.free()
        if failed:
            raise RuntimeError("ShardedRaht(direct=True): a direct gather timed out waiting for a peer; results since then are not valid")

    def _gather_roots(self, bs, which):
        """the all-gathers of one direction (one buffer set; mixed precision: the float and the wide one), timed as one"""
        timed = self._ev is not None and bs[0].send.is_cuda
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        for b in bs:
            if self._direct_failed and b.exchange is not None:
                raise RuntimeError("ShardedRaht(direct=True): an earlier direct gather timed out waiting for a peer; the ranks are out of "
                                   "phase and the double buffers no longer mean anything -- rebuild the object (or use the RCCL path)")
            b.gather(self.coll)
        if timed:
            e1.record()
            self._ev[which].append((e0, e1))

    def gathered_bytes_per_step(self, D, elem=4):
        """bytes every rank receives per direction x 2 directions (n_wide > 0: + the wide roots' float64 gathers)"""
        if self.world == 1:
            return 0
        return 2 * self.gather_rows * (D * elem + self.n_wide * 8)

    # ---- transforms ------------------------------------------------------------------------------
    def _top_forward(self, bs):
        self._gather_roots(bs, "fwd")
        for b in bs:
            self.top.forward(b.recv, want_w=False, out=b.res)

    def _top_inverse(self, bs):
        self._gather_roots(bs, "inv")
        for b in bs:
            self.top.inverse(b.recv, out=b.res)

    # A rank without rows (self.plan is None) has nothing to transform but still enters both collectives: every
    # method below reaches _top_forward / _top_inverse whatever N is.
    def forward(self, C):
        """-> T_local: every row holds its coefficient of the WHOLE scene's RAHT."""
        b = self._buffers(C.shape[1], C.dtype)
        T = self.plan.forward(C, want_w=False, roots=b.send_roots) if self.plan is not None else torch.empty_like(C)
        self._top_forward((b,))
        if self.n_roots:
            self.ops.rows_scatter(b.mine, self.root_rows, T)
        return T

    def inverse(self, T):
        b = self._buffers(T.shape[1], T.dtype)
        if self.n_roots:
            self.ops.rows_gather(T, self.root_rows, b.send_roots)
        self._top_inverse((b,))
        return self.plan.inverse(T, roots=b.mine) if self.plan is not None else torch.empty_like(T)

    # The shard-local fused passes of a quantized step: the plan's own for one lane, local_ops' mixed ones for two (the
    # wide columns in float64, their roots through the wide lane's buffers).
    def _local_forward_quant(self, bs, C, step):
        if self.n_wide:
            return self.ops.forward_quant_mixed(self.plan, C, step, self.n_wide, roots=bs[0].send_roots, roots_wide=bs[1].send_roots)
        return self.plan.forward_quant(C, step, roots=bs[0].send_roots)

    def _local_dequant_inverse(self, bs, Q, step):
        if self.n_wide:
            return self.ops.dequant_inverse_mixed(self.plan, Q, step, self.n_wide, roots=bs[0].mine, roots_wide=bs[1].mine)
        return self.plan.dequant_inverse(Q, step, roots=bs[0].mine)

    def forward_quant(self, C, step):
        """-> Q_local (int32, rank-local order_RAGFT order); the top coefficients are quantized too."""
        lanes, bs = self._lanes(C.shape[1])
        Q = (self._local_forward_quant(bs, C, step) if self.plan is not None
             else torch.empty(C.shape, dtype=torch.int32, device=C.device))
        self._top_forward(bs)
        if self.n_roots:
            pos = self._root_positions()
            for lane, st in zip(lanes, self._lane_steps(step, C.shape[1])):
                lane.quant(lane.mine_cols, st, pos, Q if lane.cols is None else Q[:, lane.cols])
        return Q

    def dequant_inverse(self, Q, step):
        lanes, bs = self._lanes(Q.shape[1])
        if self.n_roots:
            pos = self._root_positions()
            for lane, st in zip(lanes, self._lane_steps(step, Q.shape[1])):
                lane.dequant(Q if lane.cols is None else Q[:, lane.cols], st, pos, lane.send_cols)
        self._top_inverse(bs)
        if self.plan is None:
            return torch.empty(Q.shape, dtype=self.qdt, device=Q.device)
        return self._local_dequant_inverse(bs, Q, step)

    # ---- bench helpers -----------------------------------------------------------------------------
    def step(self, C, quant_step=None):
        if quant_step is None:
            return self.inverse(self.forward(C))
        return self.dequant_inverse(self.forward_quant(C, quant_step), quant_step)

    def local_step(self, C, quant_step=None):
        """The shard-local part of step() alone (bench.py: what is left of a step without the exchange): truncated
        forward (+ quantize) and (dequantize +) inverse, roots through the send / result buffers, NO collective and
        no top tree. Its output is not a transform of anything; it exists to be timed."""
        if self.plan is None:
            return None
        if quant_step is None:
            b = self._buffers(C.shape[1], C.dtype)
            return self.plan.inverse(self.plan.forward(C, want_w=False, roots=b.send_roots), roots=b.mine)
        bs = self._lanes(C.shape[1])[1]
        return self._local_dequant_inverse(bs, self._local_forward_quant(bs, C, quant_step), quant_step)

    def top_only(self, D, dtype=torch.float32):
        """The replicated top tree of both directions on whatever the buffers hold (bench.py: timed alone)."""
        b = self._buffers(D, dtype)
        self.top.forward(b.recv, want_w=False, out=b.res)
        self.top.inverse(b.recv, out=b.res)

    def roundtrip_error(self, C):
        R = self.inverse(self.forward(C))
        if self.direct:
            self.check_exchange()
        if self.N == 0:
            return 0.0
        return float(((R - C).abs().max() / C.abs().max()).item())

    def _gather_var(self, x):
        """one-off (verification): all-gather row blocks of different heights -> the concatenation in rank order"""
        if self.world == 1:
            return x
        n = self._all_gather(torch.tensor([[x.shape[0]]], dtype=torch.int64, device=x.device)).reshape(-1).tolist()
        m = int(max(n))
        pad = torch.zeros((m, x.shape[1]), dtype=x.dtype, device=x.device)
        pad[: x.shape[0]] = x
        allp = self._all_gather(pad)
        return torch.cat([allp[r * m: r * m + int(n[r])] for r in range(self.world)], dim=0)

    # ---- verification gates (not on the timed path) ------------------------------------------------
    def _gather_scene(self, C, keys_sorted):
        """-> (the whole scene's keys, the whole scene's rows of C, the number of rows on the ranks before this one)"""
        keys = self.plan_keys() if keys_sorted is None else keys_sorted
        allk = self._gather_var(keys.reshape(-1, 1).to(torch.int64)).reshape(-1).contiguous()
        allC = self._gather_var(C)
        if self.world == 1:
            return allk, allC, 0
        counts = self._all_gather(torch.tensor([[self.N]], dtype=torch.int64, device=C.device)).reshape(-1)
        return allk, allC, int(counts[: self.rank].sum().item())

    def _agree(self, out, device):
        """-> out, its "ok" only if the direct exchange met all its peers as well, and only if it is so on every rank"""
        if self.direct:
            st = self.exchange_status()
            out["direct_exchange_status"] = st
            out["ok"] = out["ok"] and st == 0
        if self.world > 1:
            flag = torch.tensor([[1 if out["ok"] else 0]], dtype=torch.int64, device=device)
            out["ok"] = bool(self._all_gather(flag).min().item() == 1)
        return out

    def check_against_unsharded(self, C, quant_step=None, keys_sorted=None):
        """Correctness gate for a multi-rank run (not on the timed path): gather the whole scene, transform it
        UNSHARDED on this rank, and compare this rank's rows with what the sharded path produced.
        float32: |dT| <= 4e-6 * column max (two float32 transforms, each within SURVEY 8c's 2e-6 of the float64 one: triangle
        inequality; measured 0.0 -- the replicated top tree performs the same butterflies on the same operands); integers: the same
        coefficient-error bound as bench.py's oracle gate."""
        allk, allC, n_before = self._gather_scene(C, keys_sorted)
        full = self.ops.make_plan(allk, self.nbits)
        Tf = full.forward(allC, want_w=False)
        mine = slice(n_before, n_before + self.N)
        T = self.forward(C)
        colmax = Tf.abs().amax(dim=0).clamp_min(1e-30)
        rel = float(((T - Tf[mine]).abs().amax(dim=0) / colmax).max().item()) if self.N else 0.0
        out = {"kind": "sharded == unsharded (whole scene gathered and transformed on every rank)", "rows_total": int(allk.shape[0]),
               "max_rel_err_T_vs_unsharded": rel, "ok": rel <= 4e-6}
        if quant_step is not None:
            Q = self.forward_quant(C, quant_step)
            R = self.dequant_inverse(Q, quant_step)
            if self.N:
                Tq = torch.empty_like(T)
                Tq[self.plan.order_RAGFT] = Q.to(T.dtype) * quant_step
                # dequantized integers sit within half a step (+ the coefficient error) of the unsharded coefficients
                worst = float(((Tq - Tf[mine]).abs() - 4e-6 * colmax).max().item())
                out["max_dequantized_distance_over_step"] = worst / quant_step
                out["ok"] = out["ok"] and worst <= 0.5 * quant_step * 1.0001
                out["quantized_roundtrip_max_err_over_step"] = float((R - C).abs().max().item()) / quant_step
        return self._agree(out, C.device)

    def check_mixed_against_unsharded(self, C, steps, keys_sorted=None):
        """Correctness gate of the mixed-precision step (n_wide > 0; not on the timed path): gather the whole scene, run the
        UNSHARDED ``forward_quant_mixed`` on it on this rank, and compare this rank's integers with the sharded
        ``forward_quant``'s, in row order, EXACTLY, on every column (the replicated top trees perform the same butterflies on
        the same operands in the same precision as the unsharded kernels; the top rows are quantized with the same arithmetic)."""
        if not self.n_wide:
            raise ValueError("check_mixed_against_unsharded needs ShardedRaht(n_wide > 0)")
        allk, allC, n_before = self._gather_scene(C, keys_sorted)
        full = self.ops.make_plan(allk, self.nbits)
        Qf = self.ops.forward_quant_mixed(full, allC, steps, self.n_wide)
        Q = self.forward_quant(C, steps)
        D = int(C.shape[1])
        out = {"kind": "sharded mixed == unsharded mixed (whole scene gathered, integers compared in row order)",
               "rows_total": int(allk.shape[0]), "n_wide": self.n_wide}
        if self.N:
            mine = Qf[full.inv_order.to(Qf.device)][n_before: n_before + self.N]      # the whole scene's integers of this rank's rows
            Qr = Q[self.plan.inv_order.to(Q.device)]
            diff = (Qr != mine)
            per_col = diff.sum(dim=0).tolist()
        else:
            per_col = [0] * D
        out["mismatches_per_column"] = [int(x) for x in per_col]
        out["mismatches"] = int(sum(per_col))
        out["ok"] = out["mismatches"] == 0
        return self._agree(out, C.device)

    def plan_keys(self):
        if self.plan is None:
            return torch.empty(0, dtype=torch.int64, device=self.device)
        ks = getattr(self.plan, "keys_tensor", None)
        if ks is None:
            raise ValueError("pass keys_sorted")
        return ks()


# ---------------------------------------------------------------------------------------------------
# front end for un-partitioned input: all-to-all by Morton prefix + local voxelizer
# ---------------------------------------------------------------------------------------------------
def exchange_by_prefix(PC, J, prefix_bits=9, vmin=None, width=None, group=None, local_ops=None):
    """Every rank holds an ARBITRARY part of the cloud: PC (n_r, 3 + d) float32, positions first. Returns this
    rank's Morton-prefix shard, voxelized: (PCvox (Nvox_r, 3 + d), keys (Nvox_r,) sorted unique int64, info).

    The concatenation of the shards over the ranks equals what the single-GPU voxelizer
    (``voxelize_pc_batched``, reference python/voxelize_pc.py:62-172) produces for the concatenation of the
    inputs in rank order, bit for bit: the bounding box is global, every voxel's points end up on one rank in
    their global order (the all-to-all delivers source ranks in order, the radix sort is stable), and the
    per-voxel mean is sequential in that order."""
    lops = local_ops or HipLocalOps
    coll = _Collectives(group)
    world, dev = coll.world, PC.device
    allreduce = coll.all_reduce if world > 1 else (lambda t, op: t)

    # ---- global bounding box (voxelize_pc.py:87-95: per-axis minimum, ONE scalar width = max extent) ----
    xyz = PC[:, :3]
    if vmin is None:
        lo = xyz.amin(dim=0) if PC.shape[0] else torch.full((3,), float("inf"), device=dev)
        vmin_t = allreduce(lo.clone(), "MIN")
    else:
        vmin_t = torch.as_tensor(vmin, dtype=torch.float32, device=dev)
    if width is None:
        hi = (xyz - vmin_t).amax() if PC.shape[0] else torch.tensor(float("-inf"), device=dev)
        width = float(allreduce(hi.reshape(1).clone(), "MAX").item())
    vmin_l = [float(v) for v in vmin_t.tolist()]
    nbits = 3 * J
    # ---- keys, 2^prefix_bits-bin population histogram, balanced prefix cuts (same on every rank) ----
    keys = lops.voxel_keys(PC, vmin_l, width, J)
    nb = 1 << prefix_bits
    pref = (keys >> (nbits - prefix_bits)).clamp(0, nb - 1) if nbits > prefix_bits else keys.clamp(0, nb - 1)
    hist = allreduce(torch.bincount(pref, minlength=nb), "SUM")
    cuts = cuts_from_histogram(hist, world)                  # rank r owns prefixes [cuts[r], cuts[r+1])
    info = {"vmin": vmin_t, "width": width, "voxel_size": width / (1 << J), "prefix_cuts": cuts, "N_global": int(hist.sum().item())}
    if world == 1:
        mine = PC
    else:
        # ---- bucket the points by destination rank (stable), ONE all-to-all of the rows ----
        dest = torch.bucketize(pref, torch.tensor(cuts[1:-1], dtype=pref.dtype, device=dev), right=True)
        _, perm = lops.sort_keys(dest, max(1, (world - 1).bit_length()))     # stable: keeps the local order per bucket
        send = torch.empty_like(PC)
        lops.rows_gather(PC, perm, send)
        mine, info["sent_rows"], info["received_rows"] = coll.all_to_all_rows(send, torch.bincount(dest, minlength=world))
    if mine.shape[0] == 0:
        return mine, torch.empty(0, dtype=torch.int64, device=dev), info
    PCvox, vkeys, _, vinfo = lops.voxelize(mine, vmin_l, width, J)
    info["Nvox_local"] = int(PCvox.shape[0])
    return PCvox, vkeys, info
