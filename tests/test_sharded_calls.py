"""What a step of ShardedRaht ENQUEUES, call by call (the contract of raht_3dgs_codec_amd/sharded.py's docstring): per direction
one shard-local call, the gathers, the top-tree launches and the row quantizer calls, in that order and nothing else; mixed
precision (n_wide = 3): float gather then wide gather, float top tree then wide top tree, quant_rows on columns [3, D) then
quant_rows_f64 on [0, 3), and the inverse in the mirrored places.

Recorded: every local_ops call, every method called on sh.plan / sh.top, every all_gather_into_tensor. CPU only: the
arithmetic is tests/numpy_mixed_ops.py's; what the recorded calls do inside themselves is not part of the sequence."""
import numpy as np
import pytest
import torch

from tests.numpy_mixed_ops import NumpyMixedLocalOps
from tests.numpy_ops import NumpyPlan
from tests.rank_procs import _cpu_barrier, run_ranks

D, NW, STEP = 7, 3, 0.01
LOG, _depth = [], [0]


def _recorded(fn, entry):
    """fn, leaving entry(*args) in LOG when called from outside any other recorded call"""
    def call(*args, **kw):
        if _depth[0] == 0:
            LOG.append(entry(*args))
        _depth[0] += 1
        try:
            return fn(*args, **kw)
        finally:
            _depth[0] -= 1
    return call


def _cols(M):
    """(first column, columns) of a column slice of a row-contiguous matrix"""
    return (M.storage_offset() % M.stride(0) if M.shape[0] else None, M.shape[1])


class RecordingPlan(NumpyPlan):
    tag = "plan"


for _m in ("forward", "inverse", "forward_quant", "dequant_inverse"):
    # the top tree's entries say what they ran on: (columns, dtype) of the gather buffer
    setattr(RecordingPlan, _m, _recorded(getattr(NumpyPlan, _m), lambda self, X, *a, _m=_m:
                                         (f"{self.tag}.{_m}",) + ((X.shape[1], X.dtype) if self.tag == "top" else ())))


class RecordingOps(NumpyMixedLocalOps):
    @staticmethod
    def make_plan(keys, nbits, top_level=None, leaf_weights=None):
        plan = RecordingPlan(keys, nbits, top_level=top_level, leaf_weights=leaf_weights)
        plan.tag = "plan" if leaf_weights is None else "top"
        return plan


for _f in ("forward_quant_mixed", "dequant_inverse_mixed", "rows_gather", "rows_scatter"):
    setattr(RecordingOps, _f, staticmethod(_recorded(getattr(NumpyMixedLocalOps, _f), lambda *a, _f=_f: (_f,))))
for _f in ("quant_rows", "quant_rows_f64"):                                 # (X, step, pos, Q): which columns of Q
    setattr(RecordingOps, _f, staticmethod(_recorded(getattr(NumpyMixedLocalOps, _f), lambda X, step, pos, Q, _f=_f: (_f,) + _cols(Q))))
for _f in ("dequant_rows", "dequant_rows_f64"):                             # (Q, step, pos, out)
    setattr(RecordingOps, _f, staticmethod(_recorded(getattr(NumpyMixedLocalOps, _f), lambda Q, step, pos, out, _f=_f: (_f,) + _cols(Q))))

F64 = torch.float64


def gather(cols):
    return ("all_gather", cols, F64)


def expected(has_rows):
    """the seven sequences; a rank without rows issues no local call but the same gathers and top-tree launches"""
    loc = (lambda *e: list(e)) if has_rows else (lambda *e: [])
    top = lambda d, *cols: [(f"top.{d}", c, F64) for c in cols]                     # noqa: E731
    return {
        "forward": loc(("plan.forward",)) + [gather(D)] + top("forward", D) + loc(("rows_scatter",)),
        "inverse": loc(("rows_gather",)) + [gather(D)] + top("inverse", D) + loc(("plan.inverse",)),
        "forward_quant": loc(("plan.forward_quant",)) + [gather(D)] + top("forward", D) + loc(("quant_rows", 0, D)),
        "dequant_inverse": loc(("dequant_rows", 0, D)) + [gather(D)] + top("inverse", D) + loc(("plan.dequant_inverse",)),
        "forward_quant_mixed": (loc(("forward_quant_mixed",)) + [gather(D), gather(NW)] + top("forward", D, NW)
                                + loc(("quant_rows", NW, D - NW), ("quant_rows_f64", 0, NW))),
        "dequant_inverse_mixed": (loc(("dequant_rows", NW, D - NW), ("dequant_rows_f64", 0, NW)) + [gather(D), gather(NW)]
                                  + top("inverse", D, NW) + loc(("dequant_inverse_mixed",))),
        "local_step": (loc(("plan.forward",), ("plan.inverse",)), loc(("plan.forward_quant",), ("plan.dequant_inverse",)),
                       loc(("forward_quant_mixed",), ("dequant_inverse_mixed",))),
    }


def _sequences(rank, world, prefix_range):
    """body of one rank: run the seven entries, -> (whether the rank owns rows, what each one enqueued)"""
    import torch.distributed as dist
    from raht_3dgs_codec_amd import sharded, synth
    real = dist.all_gather_into_tensor
    dist.all_gather_into_tensor = _recorded(real, lambda out, x, **kw: ("all_gather", x.shape[1], x.dtype))
    try:
        _, keys, C = synth.scene(600, 5, D, seed=13, prefix_range=prefix_range)
        pref = (keys >> np.uint64(15 - 9)).astype(np.int64)
        mine = np.nonzero(pref * world // 512 == rank)[0]                       # rank r: its share of the 512 prefixes
        k = torch.from_numpy(keys[mine].view(np.int64).copy())
        Cd = torch.from_numpy(C[mine].astype(np.float64))
        sh = {nw: sharded.ShardedRaht(k, 15, prefix_bits=9, local_ops=RecordingOps, force_collectives=True, n_wide=nw) for nw in (0, NW)}
        assert mine.size == 0 or sh[0].n_roots > 1, "several prefix nodes per rank"

        def run(fn, *args):
            del LOG[:]
            res = fn(*args)
            return res, list(LOG)
        got = {}
        T, got["forward"] = run(sh[0].forward, Cd)
        _, got["inverse"] = run(sh[0].inverse, T)
        Q, got["forward_quant"] = run(sh[0].forward_quant, Cd, STEP)
        _, got["dequant_inverse"] = run(sh[0].dequant_inverse, Q, STEP)
        Q, got["forward_quant_mixed"] = run(sh[NW].forward_quant, Cd, STEP)
        _, got["dequant_inverse_mixed"] = run(sh[NW].dequant_inverse, Q, STEP)
        got["local_step"] = (run(sh[0].local_step, Cd)[1], run(sh[0].local_step, Cd, STEP)[1], run(sh[NW].local_step, Cd, STEP)[1])
        # step() is the two directions, one after the other
        assert run(sh[NW].step, Cd, STEP)[1] == got["forward_quant_mixed"] + got["dequant_inverse_mixed"]
        assert run(sh[0].step, Cd)[1] == got["forward"] + got["inverse"]
        _cpu_barrier()
        return bool(mine.size), got
    finally:
        dist.all_gather_into_tensor = real


@pytest.mark.parametrize("world,prefix_range,owners", [(1, None, [True]), (2, None, [True, True]), (2, (0, 256, 9), [True, False])])
def test_a_step_enqueues_exactly_what_the_docstring_promises(world, prefix_range, owners):
    """world 1: a one-rank gloo group with the gathers forced; world 2: two ranks, and two ranks of which one owns no row"""
    res = run_ranks(_sequences, world, prefix_range)
    assert [has_rows for has_rows, _ in res] == owners
    for rank, (has_rows, got) in enumerate(res):
        want = expected(has_rows)
        for name in want:
            assert got[name] == want[name], (rank, name, got[name])
