"""The segmented RLGR coder with 64-bit segment offsets (raht_rlgr_seg_*64, rlgr.SegmentedCoder(wide=True)): frames above the
330 M symbols at which the 32-bit offset tables refuse a shape for its worst case.

Parity is anchored on the 32-bit path: tests/test_gpu_rlgr_seg.py pins it segment by segment to the host coder, which
tests/test_rlgr.py pins byte for byte to streams made by the reference's own PyRLGR. Here: (1) on small frames the 64-bit tables give
the 32-bit path's bytes; (2) the decoder reads at offsets above 2^32 and judges an offset as the 64-bit number it is; (3) the
shapes that were refused now code, sampled segments against the host coder; (4) encode_frame(entropy="gpu") on a frame above the
limit; (5) a payload that really exceeds 4 GiB."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GB = 1 << 30


@pytest.fixture(params=[-1, 0, 2, 4], ids=["out_auto", "out_word", "out_lds", "rows_per_lane"])
def decoder_output_mode(request):
    """each of the ways the decoders' symbols leave the lanes (raht_debug_rlgr_decode_out), and the batched encoder's words /
    LDS columns: small frames never pick the LDS columns by themselves"""
    from raht_3dgs_codec_amd import _lib
    prev = _lib.lib().raht_debug_rlgr_decode_out(request.param)
    prev_e = _lib.lib().raht_debug_rlgr_encode_out(request.param)
    yield request.param
    _lib.lib().raht_debug_rlgr_decode_out(prev)
    _lib.lib().raht_debug_rlgr_encode_out(prev_e)


def _need(gb):
    """the one condition on which the large tests skip: not enough free device memory"""
    import torch
    free = torch.cuda.mem_get_info()[0]
    if free < gb * GB:
        pytest.skip(f"needs about {gb} GB of free device memory, {free / GB:.1f} GB are free")


def _cases():
    """the channels of tests/test_gpu_rlgr_seg.py (same generator, same seed)"""
    rng = np.random.default_rng(11)
    lap = lambda n, b: np.rint(rng.laplace(0, b, size=n)).astype(np.int64)          # noqa: E731
    N = 70000
    chans = [lap(N, 0.3), lap(N, 3.0), lap(N, 200.0), np.zeros(N, np.int64),                          # sparse / dense / wide / all zero
             rng.integers(-2 ** 31, 2 ** 31 - 1, size=N),                                             # escapes: |u| >= 2^32 >> k
             np.where(rng.random(N) < 0.001, lap(N, 50.0), 0),                                        # long zero runs
             np.concatenate([np.zeros(N // 2, np.int64), lap(N - N // 2, 20.0)]),                     # a run across segment borders
             np.arange(N) % 7 - 3]
    return np.stack(chans).astype(np.int32)


def _step_frames(k, N=30000, D=8, seed=5):
    """k 'quantization steps' of one frame: the same Laplacian coefficients divided by growing steps (sparser and sparser)"""
    rng = np.random.default_rng(seed)
    base = rng.laplace(0, 40.0, size=(N, D)) * np.linspace(0.2, 3.0, D)[None, :]
    return [np.floor(base / (1.0 + 1.7 * j) + 0.5).astype(np.int32) for j in range(k)]


def _offsets(sc):
    """a coder's offset table as non-negative int64 (the 32-bit table is stored in an int32 tensor)"""
    import torch
    off = sc.seg_off.to(torch.int64)
    return off if sc.wide else off & 0xffffffff


def _same_tables_and_bytes(narrow, wide):
    import torch
    assert wide.wide and not narrow.wide
    assert wide.seg_off.dtype == torch.int64 and narrow.seg_off.dtype == torch.int32
    assert wide.total == narrow.total
    assert torch.equal(wide.seg_bytes, narrow.seg_bytes)
    assert torch.equal(_offsets(wide), _offsets(narrow))
    assert torch.equal(wide.out[: wide.total], narrow.out[: narrow.total])


# ---- 1. same bytes on small frames -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flag_signed", [1, 0], ids=["signed", "unsigned"])
@pytest.mark.parametrize("row_major", [False, True], ids=["channel_major", "row_major"])
@pytest.mark.parametrize("seg_len", [64, 1000, 4096, 100000])
def test_wide_tables_give_the_narrow_paths_bytes(seg_len, row_major, flag_signed, decoder_output_mode):
    import torch
    from raht_3dgs_codec_amd import rlgr
    Qcm = torch.from_numpy(_cases()).cuda()                     # (D, N); channel 4 outgrows its slot: the exact passes run too
    D, N = Qcm.shape
    Qrm = Qcm.t().contiguous()
    Q = Qrm if row_major else Qcm
    narrow = rlgr.SegmentedCoder(N, D, seg_len, flag_signed, wide=False)
    wide = rlgr.SegmentedCoder(N, D, seg_len, flag_signed, wide=True)
    assert rlgr.SegmentedCoder(N, D, seg_len, flag_signed).wide is False        # a small frame keeps the 32-bit tables by default
    tn, tw = narrow.encode(Q), wide.encode(Q)
    assert tn == tw
    _same_tables_and_bytes(narrow, wide)
    off, lens = _offsets(wide).cpu().numpy(), wide.seg_bytes.cpu().numpy().view(np.uint32).astype(np.int64)
    assert off[0] == 0 and off[-1] == tw and np.array_equal(np.diff(off), (lens + 3) // 4 * 4)
    bn, bw = narrow.container(), wide.container()
    assert bn == bw and wide.size_bytes == len(bw) == narrow.size_bytes
    # either coder decodes its own streams and the other's container, in both output layouts
    for coder in (wide, narrow, rlgr.SegmentedCoder.from_container(bn, wide=True), rlgr.SegmentedCoder.from_container(bw, wide=False),
                  rlgr.SegmentedCoder.from_container(bw)):
        assert torch.equal(coder.decode(), Qcm) and torch.equal(coder.decode(row_major=True), Qrm)
        assert int(coder.bad.item()) == 0
    assert rlgr.SegmentedCoder.from_container(bw).wide is False


@pytest.mark.parametrize("k,seg_len,row_major", [(1, 1000, True), (3, 64, True), (12, 2048, True), (13, 4096, True), (3, 1001, False), (12, 100000, False),
                                                   (13, 333, False)])
def test_wide_batch_is_the_narrow_batch_and_every_frame_alone(k, seg_len, row_major, decoder_output_mode):
    import torch
    from raht_3dgs_codec_amd import rlgr
    frames = _step_frames(k)
    N, D = frames[0].shape
    rm = [torch.from_numpy(f).cuda() for f in frames]
    cm = [q.t().contiguous() for q in rm]
    Qs = rm if row_major else cm
    narrow = [rlgr.SegmentedCoder(N, D, seg_len, wide=False) for _ in range(k)]
    wide = [rlgr.SegmentedCoder(N, D, seg_len, wide=True) for _ in range(k)]
    assert rlgr.SegmentedCoder.encode_batch(narrow, Qs) == rlgr.SegmentedCoder.encode_batch(wide, Qs)
    for a, b, Q in zip(narrow, wide, Qs):
        _same_tables_and_bytes(a, b)
        assert a.container() == b.container()
        alone = rlgr.SegmentedCoder(N, D, seg_len, wide=True)
        alone.encode(Q)
        assert alone.total == b.total and torch.equal(alone.seg_off, b.seg_off) and torch.equal(alone.out[: alone.total], b.out[: b.total])
    for out_rm in (False, True):
        outs = rlgr.SegmentedCoder.decode_batch(wide, row_major=out_rm)
        assert all(torch.equal(o, q) for o, q in zip(outs, rm if out_rm else cm))
    assert int(wide[0].bad.item()) == 0
    # the round-trip assertion inside the decoder (row-major frames): silent on the right frames, finds an altered symbol
    outs = rlgr.SegmentedCoder.decode_batch(wide, row_major=True, expect=rm)
    assert rlgr.SegmentedCoder.roundtrip_failed(wide) == []
    assert all(torch.equal(o, q) for o, q in zip(outs, rm))
    wrong = [q.clone() for q in rm]
    wrong[k - 1][N - 1, D - 1] += 1
    wrong[0][0, 0] -= 2
    fresh = [rlgr.SegmentedCoder.from_container(b.container(), wide=True) for b in wide]
    outs = rlgr.SegmentedCoder.decode_batch(fresh, row_major=True, expect=wrong)
    assert rlgr.SegmentedCoder.roundtrip_failed(fresh) == sorted({0, k - 1})
    assert all(torch.equal(o, q) for o, q in zip(outs, rm))
    # a batch is of one width
    with pytest.raises(ValueError):
        rlgr.SegmentedCoder.encode_batch([wide[0], narrow[0]], [Qs[0], Qs[0]])
    with pytest.raises(ValueError):
        rlgr.SegmentedCoder.decode_batch([narrow[0], wide[0]])


def test_incompressible_data_through_the_wide_path():
    """full-range noise: every segment outgrows its slot (the exact passes), the stream outgrows the raw-dump estimate (the buffer
    grows from the 64-bit RAHT_ERR_NOMEM total); single frames and a batch with one such frame"""
    import torch
    from raht_3dgs_codec_amd import rlgr
    rng = np.random.default_rng(9)
    N, D = 20000, 3
    Q = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31 - 1, size=(D, N)).astype(np.int32)).cuda()
    narrow, wide = rlgr.SegmentedCoder(N, D, 1024, wide=False), rlgr.SegmentedCoder(N, D, 1024, wide=True)
    cap0 = wide.cap
    tn, tw = narrow.encode(Q), wide.encode(Q)
    assert tw == tn and tw > 4 * N * D and tw > cap0 and wide.cap >= tw
    _same_tables_and_bytes(narrow, wide)
    assert torch.equal(wide.decode(), Q) and int(wide.bad.item()) == 0
    frames = _step_frames(3, N=20000, D=6)
    frames[1] = rng.integers(-2 ** 31, 2 ** 31 - 1, size=frames[1].shape).astype(np.int32)
    Qs = [torch.from_numpy(f).cuda() for f in frames]
    bn = [rlgr.SegmentedCoder(20000, 6, 512, wide=False) for _ in frames]
    bw = [rlgr.SegmentedCoder(20000, 6, 512, wide=True) for _ in frames]
    assert rlgr.SegmentedCoder.encode_batch(bn, Qs) == rlgr.SegmentedCoder.encode_batch(bw, Qs)
    assert bw[1].total > 4 * 20000 * 6
    for a, b in zip(bn, bw):
        _same_tables_and_bytes(a, b)
    outs = rlgr.SegmentedCoder.decode_batch(bw, row_major=True)
    assert all(torch.equal(o, q) for o, q in zip(outs, Qs)) and int(bw[0].bad.item()) == 0


def test_offset_scan_of_more_blocks_than_one_launch_sums():
    """4.48 M segments: more than the 2048 x 2048 the two-launch scan takes, so the 64-bit scan recurses on its block sums. The
    shape (seg_len 64) still fits the 32-bit tables, whose scan is the yardstick."""
    import torch
    from raht_3dgs_codec_amd import rlgr
    N, D, S = 64 * 70_000, 64, 64
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    Q = torch.randint(-3, 4, (N, D), generator=g, device="cuda", dtype=torch.int32)
    Q *= (torch.rand((N, D), generator=g, device="cuda") < 0.2)
    narrow, wide = rlgr.SegmentedCoder(N, D, S, wide=False), rlgr.SegmentedCoder(N, D, S, wide=True)
    assert wide.G == 4_480_000 > 2048 * 2048 and rlgr.SegmentedCoder(N, D, S).wide is False
    assert narrow.encode(Q) == wide.encode(Q)
    _same_tables_and_bytes(narrow, wide)
    assert torch.equal(wide.decode(row_major=True), Q) and int(wide.bad.item()) == 0


# ---- 2. offsets above 2^32 on the decode side --------------------------------------------------------------------------------

def test_decoder_reads_at_offsets_above_4_gib_and_judges_the_whole_offset():
    import torch
    from raht_3dgs_codec_amd import rlgr
    rng = np.random.default_rng(21)
    N, D, S = 20000, 3, 1024
    Qh = np.rint(rng.laplace(0, 30.0, size=(D, N))).astype(np.int32)
    Qh[1] = rng.integers(-2 ** 31, 2 ** 31 - 1, size=N)
    Q = torch.from_numpy(Qh).cuda()
    sc = rlgr.SegmentedCoder(N, D, S, wide=True)
    total = sc.encode(Q)
    BIG, SHIFT = 2 ** 32 + (1 << 20), 2 ** 32 + 64
    assert total + 64 <= 1 << 20
    big = torch.zeros(BIG, dtype=torch.uint8, device="cuda")
    big[SHIFT: SHIFT + total] = sc.out[:total]
    dec = rlgr.SegmentedCoder(N, D, S, wide=True, payload_cap=16)
    dec.seg_bytes.copy_(sc.seg_bytes)
    good_off = sc.seg_off + SHIFT
    dec.seg_off.copy_(good_off)
    dec.out, dec.cap, dec.total = big, BIG, BIG                  # in_bytes = the whole buffer
    assert int(dec.seg_off.min().item()) >= 2 ** 32
    assert torch.equal(dec.decode(), Q) and torch.equal(dec.decode(row_major=True), Q.t())
    assert int(dec.bad.item()) == 0
    # table entries as they might come off the wire: the segment decodes as zeros, the flag is raised, its neighbours are untouched
    g = 5                                                        # channel 0, segment 5
    good_len = int(sc.seg_bytes[g].item())

    def corrupt(coder, base_off, off=None, nbytes=None):
        coder.seg_off.copy_(base_off)
        coder.seg_bytes.copy_(sc.seg_bytes)
        if off is not None:
            coder.seg_off[g] = off
        if nbytes is not None:
            coder.seg_bytes[g] = nbytes
        coder.bad.zero_()
        for rm in (False, True):
            out = coder.decode(row_major=rm)
            torch.cuda.synchronize()
            got = out.t() if rm else out
            assert int(coder.bad.item()) == 1, (off, nbytes, rm)
            assert not bool(got[0, g * S: (g + 1) * S].any()), (off, nbytes, rm)
            assert torch.equal(got[0, : g * S], Q[0, : g * S]) and torch.equal(got[0, (g + 1) * S:], Q[0, (g + 1) * S:])
            assert torch.equal(got[1:], Q[1:])

    at = int(good_off[g].item())
    corrupt(dec, good_off, off=BIG + 4)                          # past in_bytes
    corrupt(dec, good_off, off=at + 2)                           # not 4-byte aligned
    corrupt(dec, good_off, nbytes=(1 << 20) + 4096)              # a length that reaches past the end
    corrupt(dec, good_off, nbytes=-1)                            # 2^32 - 1 bytes: its padded length must not wrap to 0
    corrupt(dec, good_off, off=2 ** 33 + at)                     # far past the end, low bits those of a valid offset
    # a buffer SMALLER than 4 GiB: a valid offset plus 2^32 has valid low 32 bits -- a decoder that narrowed the offset before it
    # checked would decode the right symbols and say nothing
    assert good_len > 0 and sc.total < 2 ** 32
    small_off = sc.seg_off.clone()
    corrupt(sc, small_off, off=int(small_off[g].item()) + 2 ** 32)
    corrupt(sc, small_off, off=int(small_off[g].item()) + 2 ** 32 + 2 ** 40)
    sc.seg_off.copy_(small_off)
    sc.bad.zero_()
    assert torch.equal(sc.decode(), Q) and int(sc.bad.item()) == 0


# ---- 3. the refused shapes now code --------------------------------------------------------------------------------------------

_BIG = {}


def _laplacian_frame(N, D, seed, div=1.0):
    """(N, D) int32 built on the device: Laplacian magnitudes, scale per channel (as _step_frames), divided by a 'step'"""
    import torch
    key = (N, D, seed, div)
    if key not in _BIG:
        _BIG.clear()
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        scale = 40.0 * torch.linspace(0.2, 3.0, D, device="cuda") / div
        Q = torch.empty((N, D), dtype=torch.int32, device="cuda")
        for lo in range(0, N, 500_000):
            n = min(500_000, N - lo)
            u = torch.rand((n, D), generator=g, device="cuda") - 0.5
            lap = -torch.sign(u) * torch.log1p(-(2.0 * u.abs()).clamp_(max=1.0 - 1e-7))
            Q[lo: lo + n] = torch.floor(lap * scale + 0.5).to(torch.int32)
        _BIG[key] = Q
    return _BIG[key]


def _segments_equal_the_host_coder(sc, Q, row_major, pairs):
    from raht_3dgs_codec_amd import rlgr
    S = sc.S
    for c, s in pairs:
        sl = (Q[s * S: (s + 1) * S, c] if row_major else Q[c, s * S: (s + 1) * S]).contiguous().cpu().numpy()
        m = rlgr.membuf()
        m.rlgrWrite(sl, sc.flag)
        assert np.array_equal(sc.segment(c, s), m.get_array()), (c, s)


def _sample_pairs(sc, n, seed):
    rng = np.random.default_rng(seed)
    pairs = {(0, 0), (0, sc.nseg - 1), (sc.D - 1, 0), (sc.D - 1, sc.nseg - 1)}
    pairs |= {(int(c), int(s)) for c, s in zip(rng.integers(0, sc.D, n), rng.integers(0, sc.nseg, n))}
    return sorted(pairs)


@pytest.mark.parametrize("seg_len", [2048, 1024])
@pytest.mark.parametrize("row_major", [True, False], ids=["row_major", "channel_major"])
def test_a_6m_x_56_frame_codes_with_the_default_arguments(row_major, seg_len):
    import torch
    from raht_3dgs_codec_amd import _lib, rlgr
    _need(8)
    N, D = 6_000_000, 56
    Qrm = _laplacian_frame(N, D, seed=31)
    Q = Qrm if row_major else Qrm.t().contiguous()
    with pytest.raises(_lib.RahtError, match="4 GiB"):                          # the 32-bit tables still refuse it
        rlgr.SegmentedCoder(N, D, seg_len, wide=False).encode(Q)
    sc = rlgr.SegmentedCoder(N, D, seg_len)
    assert sc.wide is True and sc.seg_off.dtype == torch.int64
    total = sc.encode(Q)
    lens = sc.seg_bytes.to(torch.int64) & 0xffffffff
    assert int(sc.seg_off[0].item()) == 0 and int(sc.seg_off[-1].item()) == total == sc.total
    assert torch.equal(sc.seg_off[1:] - sc.seg_off[:-1], (lens + 3) // 4 * 4)
    print(f"[rlgr_wide] {N} x {D} seg_len {seg_len} {'row' if row_major else 'channel'}-major: {total} payload bytes, {8.0 * total / (N * D):.3f} bits per symbol")
    back = sc.decode(row_major=True)
    assert torch.equal(back, Qrm) and int(sc.bad.item()) == 0
    del back
    back = sc.decode(row_major=False)
    assert torch.equal(back.t(), Qrm) and int(sc.bad.item()) == 0
    del back
    pairs = _sample_pairs(sc, 220, seed=seg_len + int(row_major))
    assert len(pairs) >= 204
    _segments_equal_the_host_coder(sc, Q, row_major, pairs)


@pytest.mark.parametrize("row_major,seg_len", [(True, 2048), (False, 1024)], ids=["row_major-2048", "channel_major-1024"])
def test_a_batch_of_three_6m_x_56_frames_is_the_three_single_encodes(row_major, seg_len):
    import torch
    from raht_3dgs_codec_amd import rlgr
    _need(24)
    N, D = 6_000_000, 56
    base = _laplacian_frame(N, D, seed=31)
    Qs = [base, torch.div(base, 3, rounding_mode="trunc"), torch.div(base, 7, rounding_mode="trunc")]    # sparser and sparser
    _BIG.clear()
    if not row_major:
        Qs = [q.t().contiguous() for q in Qs]
    batch = [rlgr.SegmentedCoder(N, D, seg_len) for _ in Qs]
    assert all(c.wide for c in batch)
    totals = rlgr.SegmentedCoder.encode_batch(batch, Qs)
    for c, Q, t in zip(batch, Qs, totals):
        alone = rlgr.SegmentedCoder(N, D, seg_len)
        assert alone.encode(Q) == t == c.total
        assert torch.equal(alone.seg_bytes, c.seg_bytes) and torch.equal(alone.seg_off, c.seg_off)
        assert torch.equal(alone.out[:t], c.out[:t])
        del alone
    outs = rlgr.SegmentedCoder.decode_batch(batch, row_major=row_major, expect=Qs if row_major else None)
    assert all(torch.equal(o, q) for o, q in zip(outs, Qs))
    if row_major:
        assert rlgr.SegmentedCoder.roundtrip_failed(batch) == []
    assert int(batch[0].bad.item()) == 0


# ---- 4. encode_frame on a frame above the limit ------------------------------------------------------------------------------

def test_encode_frame_with_the_gpu_entropy_stage_above_the_old_limit(monkeypatch):
    import torch
    from raht_3dgs_codec_amd import pipeline, rlgr, synth
    _need(12)
    _BIG.clear()
    torch.cuda.empty_cache()
    J, D = 12, 56
    Vn, keys, Cn = synth.scene(6_000_000, J, D, seed=11)
    N = Vn.shape[0]
    assert N >= 5_894_145, N                                     # the first N refused at D = 56, seg_len 2048
    V, A = torch.from_numpy(Vn.astype(np.int64)), torch.from_numpy(Cn)
    made = []
    init = rlgr.SegmentedCoder.__init__

    def spy(self, *a, **kw):
        init(self, *a, **kw)
        made.append(self)

    monkeypatch.setattr(rlgr.SegmentedCoder, "__init__", spy)
    steps = [0.05, 0.1, 0.2]
    host = pipeline.encode_frame(V, A, J, steps[:1], dtype=torch.float32, fused=True)
    gpu = pipeline.encode_frame(V, A, J, steps[:1], dtype=torch.float32, fused=True, entropy="gpu")
    assert len(made) == 1 and made[0].wide is True and (made[0].N, made[0].D, made[0].S) == (N, D, 2048)
    assert gpu[0]["size_bytes"] == made[0].size_bytes == 8 + 40 + 4 * made[0].G + made[0].total
    assert torch.equal(host[0]["C_rec"], gpu[0]["C_rec"])         # both entropy stages are lossless around the same integers
    for k in ("PSNR_all", "PSNR_quats", "PSNR_scales", "PSNR_opacity", "PSNR_colors"):
        assert host[0][k] == gpu[0][k], k
    assert host[0]["size_bytes"] <= gpu[0]["size_bytes"] <= 1.02 * host[0]["size_bytes"] + 4 * made[0].G + 2048
    first = gpu[0]["size_bytes"]
    del host, gpu
    made.clear()
    torch.cuda.empty_cache()
    one = pipeline.encode_frame(V, A, J, steps, dtype=torch.float32, fused=True, entropy="gpu", keep_rec=False)
    made.clear()
    torch.cuda.empty_cache()
    allb = pipeline.encode_frame(V, A, J, steps, dtype=torch.float32, fused=True, entropy="gpu", keep_rec=False, batch_steps=True)
    assert len(made) == 3 and all(c.wide for c in made)
    assert [r["size_bytes"] for r in one] == [r["size_bytes"] for r in allb] and one[0]["size_bytes"] == first
    assert all(r["Batched_steps"] == 3 for r in allb)
    for a, b in zip(one, allb):
        for k in ("PSNR_all", "PSNR_quats", "PSNR_scales", "PSNR_opacity", "PSNR_colors"):
            assert a[k] == b[k], k


# ---- 5. a payload that really exceeds 4 GiB ---------------------------------------------------------------------------------------

def test_a_payload_of_more_than_4_gib():
    """280 M x 4 symbols of full-range noise: no lossless code averages under 32 bits per symbol on it, so the payload is at least
    4.48e9 bytes > 2^32 -- the 64-bit scan crosses the boundary, the RAHT_ERR_NOMEM total is a 64-bit one (the raw-dump estimate is
    too small for the ~33 bits RLGR spends per such symbol), and the exact two-pass encoder writes at offsets above 2^32."""
    import torch
    from raht_3dgs_codec_amd import rlgr
    _need(32)
    _BIG.clear()
    torch.cuda.empty_cache()
    N, D, S = 280_000_000, 4, 2048
    g = torch.Generator(device="cuda")
    g.manual_seed(55)
    Q = torch.empty((D, N), dtype=torch.int32, device="cuda")
    for c in range(D):
        for lo in range(0, N, 70_000_000):
            Q[c, lo: lo + 70_000_000] = torch.randint(-2 ** 31, 2 ** 31, (70_000_000,), generator=g, device="cuda", dtype=torch.int64).to(torch.int32)
    sc = rlgr.SegmentedCoder(N, D, S)
    assert sc.wide is True
    cap0 = sc.cap
    if cap0 >= 4.6e9:                                            # (never with the default estimate: 4 N D + 64 G = 4.515e9)
        sc = rlgr.SegmentedCoder(N, D, S, payload_cap=2 ** 32 + 4096)
        cap0 = sc.cap
    total = sc.encode(Q)
    print(f"[rlgr_wide] {N} x {D} noise: {total} payload bytes, {8.0 * total / (N * D):.3f} bits per symbol, cap {cap0} -> {sc.cap}")
    assert total > 2 ** 32
    assert total > cap0 and sc.cap >= total                      # the buffer grew, from a total above 2^32
    lens = sc.seg_bytes.to(torch.int64) & 0xffffffff
    assert sc.seg_off.dtype == torch.int64 and int(sc.seg_off[0].item()) == 0 and int(sc.seg_off[-1].item()) == total
    assert torch.equal(sc.seg_off[1:] - sc.seg_off[:-1], (lens + 3) // 4 * 4)
    back = sc.decode()
    assert torch.equal(back, Q) and int(sc.bad.item()) == 0
    del back
    g0 = int(torch.searchsorted(sc.seg_off[:-1].contiguous(), torch.tensor([2 ** 32], device="cuda")).item())    # first offset >= 2^32
    assert 1 <= g0 < sc.G - 8 and int(sc.seg_off[g0].item()) >= 2 ** 32 > int(sc.seg_off[g0 - 1].item())
    rng = np.random.default_rng(77)
    gs = sorted({g0 - 2, g0 - 1, g0, g0 + 1} | set(range(sc.G - 8, sc.G)) | {int(x) for x in rng.integers(0, sc.G, 50)})
    assert sum(int(sc.seg_off[x].item()) >= 2 ** 32 for x in gs) >= 10
    _segments_equal_the_host_coder(sc, Q, False, [divmod(x, sc.nseg) for x in gs])
