"""Mixed precision on truncated plans (csrc/transform_mx.hip with the two root buffers: raht_plan_set_root_buffer +
raht_plan_set_root_buffer_wide): two and three Morton-prefix shards emulated on one GPU, as
test_gpu_parity.py::test_two_prefix_shards_stitched_by_the_top_stage does for the float32 transform.

Per shard: the wide roots are bit-identical to the float64 transform's roots, the float roots' columns [n_wide, D) to the
float32 fused forward's, the non-root Q rows to raht_fwd_quant (columns [n_wide, D)) and raht_fwd_quant_f64 ([0, n_wide)).
Stitched by a weighted top tree (float32 on the float roots, float64 on the wide ones, the top rows quantized by
quant_rows / quant_rows_f64), the integers and the reconstruction equal the UNSHARDED mixed kernels' exactly. Covered: a tile
stage last, the top kernel last, one-stage trees (tile and top kernel), and the two-pass path (D - n_wide < 4; level engine)."""
import numpy as np
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


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# name: (J, draws, D, n_wide, engine (set_engine arguments), prefix cuts, expected schedule)
CASES = {
    "tile_last_2":   (9, 90000, 59, 3, ("tile", 0, 0, 0, 1), [200], "tile_last"),
    "tile_last_3":   (9, 90000, 59, 3, ("tile", 128, 64, 0, 1), [150, 330], "tile_last"),
    "top_last_2":    (9, 90000, 59, 3, ("tile", 0, 0, 0, 8192), [260], "top_last"),
    "top_last_3":    (9, 90000, 59, 2, ("tile", 256, 128, 0, 4096), [100, 400], "top_last"),
    "one_top_stage": (6, 6000, 59, 3, ("tile", 0, 0, 0, 8192), [250], "one_stage"),
    "one_tile_stage": (5, 800, 59, 3, ("tile", 512, 64, 0, 1), [256], "one_stage"),
    "two_pass_narrow": (9, 60000, 6, 3, ("tile",), [220], "two_pass"),
    "two_pass_level": (9, 60000, 59, 3, ("level",), [120, 300], "two_pass"),
}
STEPS = [0.01, 1.0, "per_channel"]


def _steps(which, D):
    return [0.01 * (1 + (c % 7)) for c in range(D)] if which == "per_channel" else which


def _split(steps, nw):
    return (steps[nw:], steps[:nw]) if isinstance(steps, list) else (steps, steps)


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_truncated_mixed_shards_stitch_to_the_unsharded_mixed_step(rt, case, step):
    import torch
    from raht_3dgs_codec_amd import ops, synth
    J, n, D, nw, engine, pcuts, sched = CASES[case]
    V, keys, C = synth.scene(n, J, D, seed=53)
    nbits, pb = 3 * J, 9
    pref = (keys >> np.uint64(nbits - pb)).astype(np.int64)
    cuts = [0] + [int(np.searchsorted(pref, c)) for c in pcuts] + [keys.shape[0]]
    shards = list(zip(cuts[:-1], cuts[1:]))
    assert all(b > a for a, b in shards)
    steps = _steps(step, D)
    sf, sw = _split(steps, nw)
    Cd = _dev(C)
    parts, roots_f, roots_w, metas = [], [], [], []
    for a, b in shards:
        pl = rt.RahtPlan.from_keys(_dev(keys[a:b].view(np.int64)), nbits, top_level=nbits - pb)
        pl.set_engine(*engine)
        st = pl.mixed_stats(D, nw)
        rows = st["rows_per_stage"]
        if sched == "two_pass":
            assert st["tile_rows"] == 0
        else:
            assert st["tile_rows"] >= 64 and rows[0] == b - a
            if sched == "one_stage":
                assert len(rows) == 1
            elif sched == "tile_last":
                assert len(rows) >= 2 and rows[-1] > engine[4]
            else:
                assert len(rows) >= 2 and rows[-1] <= engine[4]
        Cs = Cd[a:b]
        nr = pl.n_roots
        rb = torch.full((nr, D), 7.5, dtype=torch.float32, device="cuda")
        rw = torch.full((nr, nw), 7.5, dtype=torch.float64, device="cuda")
        Q = pl.forward_quant_mixed(Cs, steps, nw, roots=rb, roots_wide=rw)
        # the roots: float64 transform's on the wide columns, float32 fused forward's on the others
        rw_ref = torch.empty_like(rw)
        pl.forward(Cs[:, :nw].double().contiguous(), want_w=False, roots=rw_ref)
        assert torch.equal(rw, rw_ref), (case, step)
        rb32 = torch.empty_like(rb)
        Q32 = pl.forward_quant(Cs, steps, roots=rb32)
        assert torch.equal(rb[:, nw:], rb32[:, nw:]), (case, step)
        # the non-root rows of Q (float64 fused forward: the same plan at its default tile geometry -- the float64 tile kernels do
        # not fit every forced one)
        ref64 = rt.RahtPlan.from_keys(_dev(keys[a:b].view(np.int64)), nbits, top_level=nbits - pb)
        ref64.set_engine(*engine[:1])
        rb64 = torch.empty((nr, D), dtype=torch.float64, device="cuda")
        Q64 = ref64.forward_quant(Cs.double(), steps, roots=rb64)
        nonroot = torch.ones(b - a, dtype=torch.bool, device="cuda")
        nonroot[pl.inv_order[pl.root_rows]] = False
        assert torch.equal(Q[nonroot][:, nw:], Q32[nonroot][:, nw:]), (case, step)
        assert torch.equal(Q[nonroot][:, :nw], Q64[nonroot][:, :nw]), (case, step)
        rr = pl.root_rows.cpu().numpy()
        parts.append((pl, Q)); roots_f.append(rb); roots_w.append(rw)
        metas.append((pref[a:b][rr], np.diff(np.concatenate([rr, [b - a]]))))
    # the top tree: float32 on the float roots, float64 on the wide ones; the top rows quantized into each shard's Q
    tp = np.concatenate([m[0] for m in metas]); tc = np.concatenate([m[1] for m in metas])
    top = rt.RahtPlan.from_keys(_dev(tp.astype(np.int64)), pb, leaf_weights=_dev(tc.astype(np.int64)))
    if engine[0] == "level":
        top.set_engine("level")
    Tf = top.forward(torch.cat(roots_f), want_w=False)
    Tw = top.forward(torch.cat(roots_w), want_w=False)
    full = rt.RahtPlan.from_keys(_dev(keys.view(np.int64)), nbits)
    full.set_engine(*engine[:1])
    Qfull = full.forward_quant_mixed(Cd, steps, nw)
    Qfull_rows = Qfull[full.inv_order]
    off = 0
    for (pl, Q), (a, b) in zip(parts, shards):
        nr = pl.n_roots
        pos = pl.inv_order[pl.root_rows]
        ops.quant_rows(Tf[off: off + nr][:, nw:], sf, pos, Q[:, nw:])
        ops.quant_rows_f64(Tw[off: off + nr], sw, pos, Q[:, :nw])
        off += nr
        bad = (Q[pl.inv_order] != Qfull_rows[a:b])
        assert not bool(bad.any()), (case, step, bad.sum(dim=0).nonzero().flatten().tolist())
    # inverse: the top rows dequantized, the top tree inverted (both precisions), the shards from their root buffers
    Ctop_f, Ctop_w, off = [], [], 0
    tf_in = torch.empty_like(Tf); tw_in = torch.empty_like(Tw)
    for pl, Q in parts:
        nr = pl.n_roots
        pos = pl.inv_order[pl.root_rows]
        ops.dequant_rows(Q[:, nw:], sf, pos, out=tf_in[off: off + nr][:, nw:])
        ops.dequant_rows_f64(Q[:, :nw], sw, pos, out=tw_in[off: off + nr])
        off += nr
    Rf = top.inverse(tf_in)
    Rw = top.inverse(tw_in)
    Cfull = full.dequant_inverse_mixed(Qfull, steps, nw)
    off = 0
    for (pl, Q), (a, b) in zip(parts, shards):
        nr = pl.n_roots
        Cr = pl.dequant_inverse_mixed(Q, steps, nw, roots=Rf[off: off + nr].contiguous(), roots_wide=Rw[off: off + nr].contiguous())
        off += nr
        assert torch.equal(Cr, Cfull[a:b]), (case, step, float((Cr - Cfull[a:b]).abs().max()))


def test_truncated_mixed_refusals(rt):
    import torch
    from raht_3dgs_codec_amd import synth
    J, D, nw = 8, 59, 3
    V, keys, C = synth.scene(30000, J, D, seed=3)
    pl = rt.RahtPlan.from_keys(_dev(keys.view(np.int64)), 3 * J, top_level=3 * J - 9)
    Cd = _dev(C)
    nr = pl.n_roots
    rb = torch.zeros((nr, D), dtype=torch.float32, device="cuda")
    rw = torch.zeros((nr, nw), dtype=torch.float64, device="cuda")
    Q = pl.forward_quant_mixed(Cd, 0.01, nw, roots=rb, roots_wide=rw)
    # no buffer, or only one of the two (through the C ABI: the Python binding refuses half a pair by itself)
    with pytest.raises(rt.RahtError):
        pl.forward_quant_mixed(Cd, 0.01, nw)
    with pytest.raises(rt.RahtError):
        pl.dequant_inverse_mixed(Q, 0.01, nw)
    with pytest.raises(ValueError):
        pl.forward_quant_mixed(Cd, 0.01, nw, roots=rb)
    from raht_3dgs_codec_amd import _lib
    import ctypes
    L = _lib.lib()
    for set_f, set_w in ((True, False), (False, True)):
        if set_f:
            _lib.check(L.raht_plan_set_root_buffer(pl._h, ctypes.c_void_p(rb.data_ptr())))
        if set_w:
            _lib.check(L.raht_plan_set_root_buffer_wide(pl._h, ctypes.c_void_p(rw.data_ptr())))
        try:
            with pytest.raises(rt.RahtError):
                pl.forward_quant_mixed(Cd, 0.01, nw)
            with pytest.raises(rt.RahtError):
                pl.dequant_inverse_mixed(Q, 0.01, nw)
        finally:
            _lib.check(L.raht_plan_set_root_buffer(pl._h, None))
            _lib.check(L.raht_plan_set_root_buffer_wide(pl._h, None))
    # a row-mapped plan stays refused, with or without buffers
    tk = np.unique(np.random.default_rng(2).integers(0, 512, size=300)).astype(np.int64)
    top = rt.RahtPlan.from_keys(_dev(tk), 9)
    top.set_row_map(_dev(np.arange(tk.shape[0], dtype=np.int64) * 2), 2 * tk.shape[0])
    X = torch.zeros((2 * tk.shape[0], D), dtype=torch.float32, device="cuda")
    with pytest.raises(rt.RahtError):
        top.forward_quant_mixed(X, 0.01, nw)
    # the truncated plan's stats report its schedule
    st = pl.mixed_stats(D, nw)
    assert st["tile_rows"] >= 64 and st["rows_per_stage"][0] == keys.shape[0]


def test_f64_row_quantizers(rt):
    import torch
    from raht_3dgs_codec_amd import ops
    rng = np.random.default_rng(9)
    X = torch.from_numpy(rng.standard_normal((300, 5)) * 1e6).cuda()
    pos = torch.from_numpy(rng.permutation(1000)[:300].astype(np.int64)).cuda()
    Q = torch.zeros((1000, 8), dtype=torch.int32, device="cuda")
    steps = [0.01, 0.02, 0.5, 1.0, 3.0]
    ops.quant_rows_f64(X, steps, pos, Q[:, 2:7])
    ref = torch.floor(X / torch.tensor(steps, dtype=torch.float64, device="cuda") + 0.5).to(torch.int32)
    assert torch.equal(Q[pos][:, 2:7], ref)
    assert int((Q[:, :2] != 0).sum()) == 0 and int((Q[:, 7] != 0).sum()) == 0
    back = ops.dequant_rows_f64(Q[:, 2:7], steps, pos)
    assert back.dtype == torch.float64 and torch.equal(back, ref.double() * torch.tensor(steps, dtype=torch.float64, device="cuda"))
