"""Tile programs (csrc/schedule.hip: tile_program_kernel; raht_common.h: Stage::prog): the mixed-precision tile kernels replay every
tile's butterflies, survivors and destinations from a program built once per schedule instead of resolving them per call.

Bar: bit-identical to raht_fwd_quant_f64 / raht_dequant_inv_f64 on the wide columns and to raht_fwd_quant / raht_dequant_inv on
the others, across the program formats (compact stage-0 records, full records of later stages and weighted plans), tile
geometries from 64 to 1024 rows with ragged last tiles, truncated plans with both root buffers, and a plan used on two streams.
"""
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    _lib.lib()
    return R


def _scene(seed, N, nbits, D):
    import torch
    gen = torch.Generator(device="cuda"); gen.manual_seed(seed)
    keys = torch.unique(torch.randint(0, 1 << nbits, (int(N * 1.3) + 8,), device="cuda", dtype=torch.int64, generator=gen))[:N].contiguous()
    C = torch.randn((int(keys.shape[0]), D), device="cuda", generator=gen)
    C[:, :4] = torch.randint(0, 4096, (C.shape[0], 4), device="cuda", generator=gen).float()
    return keys, C


def _check_both_directions(p, ref, C, steps, nw, what):
    """mixed (plan p) == float64 kernels on the wide columns, float32 kernels on the others (plan `ref`: the same tree at the
    engines' default geometry -- the float64 tile kernels do not fit every forced one), forward and inverse"""
    import torch
    Q = p.forward_quant_mixed(C, steps, nw)
    Q64 = ref.forward_quant(C.double(), steps)
    Q32 = ref.forward_quant(C, steps)
    assert torch.equal(Q[:, :nw], Q64[:, :nw]), what
    assert torch.equal(Q[:, nw:], Q32[:, nw:]), what
    mixq = torch.cat([Q64[:, :nw], Q32[:, nw:]], dim=1).contiguous()
    Cr = p.dequant_inverse_mixed(mixq, steps, nw)
    C64 = ref.dequant_inverse(mixq, steps, dtype=torch.float64)
    C32 = ref.dequant_inverse(mixq, steps)
    assert torch.equal(Cr[:, :nw], C64[:, :nw].float()), what
    assert torch.equal(Cr[:, nw:], C32[:, nw:]), what
    return Q, Cr


# (n_wide, D, tile_rows, tail_rows, final_rows): compact stage-0 records at 64 .. 1024 rows, many-stage schedules (small tail
# tiles, final_rows 64), ragged last tiles (N is no multiple of any tile size)
GEOMS = [
    (1, 5, 64, 64, 64),
    (2, 14, 128, 64, 0),
    (3, 59, 0, 0, 0),
    (4, 66, 1024, 256, 0),
    (3, 32, 512, 64, 64),
    (4, 8, 1020, 1024, 0),
    (1, 63, 256, 128, 256),
    (2, 60, 64, 128, 64),
]


@pytest.mark.parametrize("geom", GEOMS)
def test_programs_match_the_runtime_resolution_engines(rt, geom):
    nw, D, r0, r1, rf = geom
    keys, C = _scene(11 + D, 150001, 36, D)
    p = rt.RahtPlan.from_keys(keys, 36)
    p.set_engine("tile", r0, r1, 0, rf)
    st = p.mixed_stats(D, nw)
    assert st["tile_rows"] >= 64 and st["rows_per_stage"][0] == C.shape[0]
    if r0:
        assert st["tile_rows"] <= r0
    if rf == 64:
        assert len(st["rows_per_stage"]) >= 3
    steps = [0.01 * (1 + (c % 7)) for c in range(D)] if D % 2 else 0.013
    _check_both_directions(p, rt.RahtPlan.from_keys(keys, 36), C, steps, nw, geom)


@pytest.mark.parametrize("geom", [(0, 0, 0), (64, 64, 64), (1024, 128, 0)])
def test_weighted_plan_takes_full_records(rt, geom):
    import torch
    keys, C = _scene(5, 60000, 30, 59)
    gen = torch.Generator(device="cuda"); gen.manual_seed(9)
    w = torch.randint(1, 50, (keys.shape[0],), device="cuda", dtype=torch.int64, generator=gen)
    p = rt.RahtPlan.from_keys(keys, 30, leaf_weights=w)
    p.set_engine("tile", geom[0], geom[1], 0, geom[2])
    assert p.mixed_stats(59, 3)["tile_rows"] >= 64
    _check_both_directions(p, rt.RahtPlan.from_keys(keys, 30, leaf_weights=w), C, 0.01, 3, geom)


def test_truncated_plan_with_both_root_buffers(rt):
    import torch
    D, nw = 59, 3
    keys, C = _scene(21, 40000, 27, D)
    p = rt.RahtPlan.from_keys(keys, 27, top_level=20)
    p.set_engine("tile", 128, 64, 0, 0)
    assert p.mixed_stats(D, nw)["tile_rows"] >= 64
    nr = p.n_roots
    rb = torch.zeros((nr, D), dtype=torch.float32, device="cuda")
    rw = torch.zeros((nr, nw), dtype=torch.float64, device="cuda")
    Q = p.forward_quant_mixed(C, 0.01, nw, roots=rb, roots_wide=rw)
    rw_ref = torch.empty_like(rw)
    p.forward(C[:, :nw].double().contiguous(), want_w=False, roots=rw_ref)
    assert torch.equal(rw, rw_ref)
    rb32 = torch.empty_like(rb)
    Q32 = p.forward_quant(C, 0.01, roots=rb32)
    assert torch.equal(rb[:, nw:], rb32[:, nw:])
    nonroot = torch.ones(C.shape[0], dtype=torch.bool, device="cuda")
    nonroot[p.inv_order[p.root_rows]] = False
    assert torch.equal(Q[nonroot][:, nw:], Q32[nonroot][:, nw:])
    # inverse from the root buffers: float32 kernel on the float columns, float64 on the wide ones
    Cr = p.dequant_inverse_mixed(Q, 0.01, nw, roots=rb, roots_wide=rw)
    C32 = p.dequant_inverse(Q32, 0.01, roots=rb32)
    assert torch.equal(Cr[:, nw:], C32[:, nw:])
    ref = rt.RahtPlan.from_keys(keys, 27, top_level=20)
    Q64 = ref.forward_quant(C.double(), 0.01, roots=torch.empty((nr, D), dtype=torch.float64, device="cuda"))
    assert torch.equal(Q[nonroot][:, :nw], Q64[nonroot][:, :nw])


def test_first_inverse_on_a_side_stream(rt):
    """A fresh plan with concurrent directions: its schedule and programs are built by a forward on the current stream and read at
    once, without a host synchronisation, by an inverse on another stream."""
    import torch
    D, nw = 59, 3
    keys, C = _scene(33, 300000, 36, D)
    ref = rt.RahtPlan.from_keys(keys, 36)
    Qref = ref.forward_quant_mixed(C, 0.01, nw)
    Cref = ref.dequant_inverse_mixed(Qref, 0.01, nw)
    torch.cuda.synchronize()
    p = rt.RahtPlan.from_keys(keys, 36)
    p.set_concurrent_directions(True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    Q = p.forward_quant_mixed(C, 0.01, nw)
    with torch.cuda.stream(side):
        Cr = p.dequant_inverse_mixed(Qref, 0.01, nw)
    torch.cuda.synchronize()
    assert torch.equal(Q, Qref)
    assert torch.equal(Cr, Cref)
