"""The ragged batch of the segmented RLGR coder (raht_rlgr_seg_encode_ragged / _decode_ragged; SegmentedCoder.encode_ragged /
decode_ragged): frames of DIFFERENT sizes through one set of launches. The bytes of a frame cannot depend on its company: every
frame's tables and container are compared with those of ``SegmentedCoder(N_j, D, seg_len).encode(Q_j)`` on its own, exactly, and a
few segments of every frame with the host coder (= the reference's, tests/test_rlgr.py) directly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# a lone symbol, a short segment, exactly one, one symbol into a second, one large frame ... and a SQUARE one (N == D), which the
# one-frame coder reads as channel-major whatever it is handed
SIZES = [1, 63, 64, 65, 70000, 129, 4096, 8]
D = 8


@pytest.fixture(params=[-1, 0, 2, 4], ids=["out_auto", "out_word", "out_lds", "rows_per_lane"], autouse=True)
def _output_mode(request):
    """every test with each of the ways the coders' words and symbols leave the lanes (raht_debug_rlgr_decode_out / _encode_out):
    these frames never reach the LDS columns by themselves"""
    from raht_3dgs_codec_amd import _lib
    prev = _lib.lib().raht_debug_rlgr_decode_out(request.param)
    prev_e = _lib.lib().raht_debug_rlgr_encode_out(request.param)
    yield
    _lib.lib().raht_debug_rlgr_decode_out(prev)
    _lib.lib().raht_debug_rlgr_encode_out(prev_e)


def _channels(N, seed):
    """(D, N) int32: the channel kinds of test_gpu_rlgr_seg._cases() at length N"""
    rng = np.random.default_rng(seed)
    lap = lambda n, b: np.rint(rng.laplace(0, b, size=n)).astype(np.int64)          # noqa: E731
    chans = [lap(N, 0.3), lap(N, 3.0), lap(N, 200.0), np.zeros(N, np.int64),                          # sparse / dense / wide / all zero
             rng.integers(-2 ** 31, 2 ** 31 - 1, size=N),                                             # escapes
             np.where(rng.random(N) < 0.001, lap(N, 50.0), 0),                                        # long zero runs
             np.concatenate([np.zeros(N // 2, np.int64), lap(N - N // 2, 20.0)]),                     # a run across segment borders
             np.arange(N) % 7 - 3]
    return np.stack(chans).astype(np.int32)


_CACHE = {}


def _reference(sizes, seg_len):
    """[(Q (D, N) numpy, seg_bytes, seg_off, payload) per frame] from one-frame encodes, computed once and left unchanged"""
    import torch
    from raht_3dgs_codec_amd import rlgr
    key = (tuple(sizes), seg_len)
    if key not in _CACHE:
        ref = []
        for j, N in enumerate(sizes):
            Q = _channels(N, 100 + j)
            sc = rlgr.SegmentedCoder(N, D, seg_len)
            total = sc.encode(torch.from_numpy(Q).cuda())
            ref.append((Q, sc.seg_bytes.cpu().numpy().copy(), sc.seg_off.cpu().numpy().copy(), sc.out[:total].cpu().numpy().copy()))
        _CACHE[key] = ref
    return _CACHE[key]


def _layout(Q, kind):
    """the (D, N) numpy matrix on the device as one of the four layouts -> the tensor view the coder is handed"""
    import torch
    d, N = Q.shape
    if kind == "rows":                                                  # row-major, sym_stride = D
        return torch.from_numpy(np.ascontiguousarray(Q.T)).cuda()
    if kind == "rows_padded":                                           # row-major, sym_stride = D + 3
        big = torch.full((N, d + 3), 12345, dtype=torch.int32, device="cuda")
        big[:, :d] = torch.from_numpy(np.ascontiguousarray(Q.T)).cuda()
        return big[:, :d]
    if kind == "chans":                                                 # channel-major, chan_stride = N (unaligned for odd N)
        return torch.from_numpy(Q).cuda()
    pad = (N + 3) // 4 * 4 + 4                                          # channel-major, chan_stride a multiple of 4
    big = torch.full((d, pad), 12345, dtype=torch.int32, device="cuda")
    big[:, :N] = torch.from_numpy(Q).cuda()
    return big[:, :N]


def _assert_same(coders, ref, what):
    for j, (c, (_, lens, offs, payload)) in enumerate(zip(coders, ref)):
        assert c.total == payload.shape[0], (what, j, c.total, payload.shape[0])
        assert np.array_equal(c.seg_bytes.cpu().numpy(), lens), (what, j)
        assert np.array_equal(c.seg_off.cpu().numpy(), offs), (what, j)                # (the closing entry seg_off[G_j] included)
        assert np.array_equal(c.out[: c.total].cpu().numpy(), payload), (what, j)


@pytest.mark.parametrize("seg_len", [64, 1000])
@pytest.mark.parametrize("kind", ["rows", "rows_padded", "chans", "chans_padded"])
def test_every_frame_gets_the_bytes_it_gets_alone(seg_len, kind):
    import torch
    from raht_3dgs_codec_amd import rlgr
    ref = _reference(SIZES, seg_len)
    Qs = [_layout(Q, kind) for Q, _, _, _ in ref]
    coders = [rlgr.SegmentedCoder(N, D, seg_len) for N in SIZES]
    totals = rlgr.SegmentedCoder.encode_ragged(coders, Qs, row_major=True if kind.startswith("rows") else None)
    assert totals == [r[3].shape[0] for r in ref]
    _assert_same(coders, ref, kind)
    # a few segments of every frame against the host coder directly
    for c, (Q, lens, offs, payload) in zip(coders, ref):
        for ch, s in {(0, 0), (2, c.nseg - 1), (4, c.nseg // 2), (D - 1, c.nseg - 1)}:
            m = rlgr.membuf()
            m.rlgrWrite(Q[ch, s * seg_len: (s + 1) * seg_len], 1)
            assert np.array_equal(c.segment(ch, s), m.get_array()), (c.N, ch, s)
    # decode: every input comes back, in both layouts, from the coders and from the wire
    wire = [rlgr.SegmentedCoder.from_container(c.container()) for c in coders]
    for cs in (coders, wire):
        for rm in (False, True):
            outs = rlgr.SegmentedCoder.decode_ragged(cs, row_major=rm)
            for o, (Q, _, _, _) in zip(outs, ref):
                want = torch.from_numpy(np.ascontiguousarray(Q.T) if rm else Q).cuda()
                assert torch.equal(o, want), (kind, rm, Q.shape)
        assert int(cs[0].bad.item()) == 0
    # ... into padded outputs: nothing outside the frames is written
    outs = [torch.full((N, D + 5), -9, dtype=torch.int32, device="cuda") for N in SIZES]
    rlgr.SegmentedCoder.decode_ragged(coders, outs=[o[:, :D] for o in outs], row_major=True)
    for o, (Q, _, _, _) in zip(outs, ref):
        assert torch.equal(o[:, :D], torch.from_numpy(np.ascontiguousarray(Q.T)).cuda()) and bool((o[:, D:] == -9).all())


@pytest.mark.parametrize("k", [1, 12, 13])
def test_batch_sizes(k):
    """one frame, the most a call takes, and one more (the wrapper's chunks)"""
    import torch
    from raht_3dgs_codec_amd import rlgr
    sizes = [SIZES[j % len(SIZES)] + 7 * (j // len(SIZES)) for j in range(k)]
    sizes = [N if N < 70000 else 9000 + N % 7 for N in sizes]
    ref = _reference(sizes, 64)
    Qs = [_layout(Q, "rows") for Q, _, _, _ in ref]
    coders = [rlgr.SegmentedCoder(N, D, 64) for N in sizes]
    rlgr.SegmentedCoder.encode_ragged(coders, Qs, row_major=True)
    _assert_same(coders, ref, k)
    outs = rlgr.SegmentedCoder.decode_ragged(coders, row_major=True, expect=Qs)
    assert all(torch.equal(o, q) for o, q in zip(outs, Qs))
    assert rlgr.SegmentedCoder.roundtrip_failed(coders) == []


def test_incompressible_frame_and_a_buffer_that_is_too_small():
    """one frame of full-range int32 among compressible ones: its segments outgrow their slots and the call goes to the exact
    passes; with one frame's `out` too small the wrapper grows it and retries. Same containers either way."""
    import torch
    from raht_3dgs_codec_amd import rlgr
    rng = np.random.default_rng(21)
    sizes = [300, 5000, 65, 2000]
    mats = [np.rint(rng.laplace(0, 4.0, size=(N, D))).astype(np.int32) for N in sizes]
    mats[1] = rng.integers(-2 ** 31, 2 ** 31 - 1, size=mats[1].shape).astype(np.int32)
    Qs = [torch.from_numpy(m).cuda() for m in mats]
    alone = []
    for N, Q in zip(sizes, Qs):
        c = rlgr.SegmentedCoder(N, D, 64)
        c.encode(Q)
        alone.append(c.container())
    coders = [rlgr.SegmentedCoder(N, D, 64) for N in sizes]
    rlgr.SegmentedCoder.encode_ragged(coders, Qs)
    assert coders[1].total > 4 * sizes[1] * D                           # the escapes cost more than a raw dump
    assert [c.container() for c in coders] == alone
    small = [rlgr.SegmentedCoder(N, D, 64, payload_cap=(64 if j == 3 else None)) for j, N in enumerate(sizes)]
    rlgr.SegmentedCoder.encode_ragged(small[2:], Qs[2:])                # compressible frames, frame 3's buffer of 64 bytes: slots pass, retry
    rlgr.SegmentedCoder.encode_ragged(small[:2], Qs[:2])
    assert small[3].cap >= small[3].total > 64
    assert [c.container() for c in small] == alone
    small = [rlgr.SegmentedCoder(N, D, 64, payload_cap=(64 if j == 0 else None)) for j, N in enumerate(sizes)]
    rlgr.SegmentedCoder.encode_ragged(small, Qs)                        # exact passes (frame 1) and a retry (frame 0) in one call
    assert [c.container() for c in small] == alone
    outs = rlgr.SegmentedCoder.decode_ragged(small, row_major=True)
    assert all(torch.equal(o, q) for o, q in zip(outs, Qs)) and int(small[0].bad.item()) == 0


def test_round_trip_assertion_and_corrupt_tables_name_their_frame():
    import torch
    from raht_3dgs_codec_amd import rlgr
    ref = _reference(SIZES, 64)
    Qs = [_layout(Q, "rows") for Q, _, _, _ in ref]
    coders = [rlgr.SegmentedCoder(N, D, 64) for N in SIZES]
    rlgr.SegmentedCoder.encode_ragged(coders, Qs, row_major=True)
    blobs = [c.container() for c in coders]
    for j, (row, col) in ((4, (69999, 3)), (0, (0, 7)), (5, (64, 0))):
        wrong = [q.clone() for q in Qs]
        wrong[j][row, col] += 1
        fresh = [rlgr.SegmentedCoder.from_container(b) for b in blobs]
        outs = rlgr.SegmentedCoder.decode_ragged(fresh, row_major=True, expect=wrong)
        torch.cuda.synchronize()
        assert int(fresh[0].bad.item()) & 0xffffffff == 1 << (16 + j)
        assert rlgr.SegmentedCoder.roundtrip_failed(fresh) == [j]
        assert all(torch.equal(o, q) for o, q in zip(outs, Qs))
    with pytest.raises(ValueError):
        rlgr.SegmentedCoder.decode_ragged(coders, row_major=False, expect=Qs)
    # a table entry of frame j outside its payload: bit j, that segment zeros, everything else intact
    for j, g in ((4, 5), (6, 70), (0, 2)):
        for rm in (True, False):
            fresh = [rlgr.SegmentedCoder.from_container(b) for b in blobs]
            fresh[j].seg_off[g] = 2 ** 31 - 4
            outs = rlgr.SegmentedCoder.decode_ragged(fresh, row_major=rm)
            torch.cuda.synchronize()
            assert int(fresh[0].bad.item()) == 1 << j
            nseg = fresh[j].nseg
            c, s = divmod(g, nseg)
            for i, (o, q) in enumerate(zip(outs, Qs)):
                o = o if rm else o.t()
                if i != j:
                    assert torch.equal(o, q), (j, g, rm, i)
                    continue
                want = q.clone()
                want[s * 64: (s + 1) * 64, c] = 0
                assert torch.equal(o, want), (j, g, rm)


def test_wrapper_refusals_and_the_same_shape_batch_keeps_its_errors():
    import torch
    from raht_3dgs_codec_amd import rlgr
    Qs = [torch.zeros((N, D), dtype=torch.int32, device="cuda") for N in (100, 200)]
    coders = [rlgr.SegmentedCoder(N, D, 64) for N in (100, 200)]
    with pytest.raises(ValueError):
        rlgr.SegmentedCoder.encode_ragged(coders, Qs[:1])
    with pytest.raises(ValueError):
        rlgr.SegmentedCoder.encode_ragged(coders, [Qs[0], Qs[1].t().contiguous()])                     # mixed layouts
    with pytest.raises(ValueError):
        rlgr.SegmentedCoder.encode_ragged([coders[0], rlgr.SegmentedCoder(200, D, 128)], Qs)          # another seg_len
    with pytest.raises(ValueError):
        rlgr.SegmentedCoder.encode_ragged([coders[0], rlgr.SegmentedCoder(200, D, 64, wide=True)], Qs)
    with pytest.raises(ValueError, match="share N, D, seg_len"):
        rlgr.SegmentedCoder.encode_batch(coders, Qs)
    with pytest.raises(ValueError, match="share N, D, seg_len"):
        rlgr.SegmentedCoder.decode_batch(coders)
    assert rlgr.SegmentedCoder.decode_ragged([]) == []


def test_a_square_frame_is_read_as_the_one_frame_coder_reads_it():
    """N == D: ``encode`` / ``decode`` of one coder read a square matrix as (D, N) channel-major. A ragged call whose layout is not
    said reads it the same way, whatever its company -- a batch of square frames only, a square frame among channel-major ones --
    and refuses it among row-major ones until ``row_major=True`` says what it is."""
    import torch
    from raht_3dgs_codec_amd import rlgr
    rng = np.random.default_rng(77)
    mats = [torch.from_numpy(np.rint(rng.laplace(0, 30.0, size=(D, D))).astype(np.int32)).cuda() for _ in range(3)]      # three different square matrices
    alone = []
    for m in mats:
        c = rlgr.SegmentedCoder(D, D, 64)
        c.encode(m)
        assert torch.equal(c.decode(), m) and torch.equal(c.decode(row_major=True), m)      # (either way the one-frame coder reads (D, N))
        alone.append(c.container())
    # square frames only
    sq = [rlgr.SegmentedCoder(D, D, 64) for _ in mats]
    rlgr.SegmentedCoder.encode_ragged(sq, mats)
    assert [c.container() for c in sq] == alone
    for o, m in zip(rlgr.SegmentedCoder.decode_ragged(sq), mats):
        assert torch.equal(o, m)                                        # (D, N), as documented
    for o, m in zip(rlgr.SegmentedCoder.decode_ragged(sq, row_major=True), mats):
        assert torch.equal(o, m.t())                                    # said to be (N, D): the transposed reading
    outs = [torch.empty_like(m) for m in mats]
    rlgr.SegmentedCoder.decode_ragged(sq, outs=outs)
    assert all(torch.equal(o, m) for o, m in zip(outs, mats))
    # the same matrices said to be row-major: the containers of their transposes
    rm = [rlgr.SegmentedCoder(D, D, 64) for _ in mats]
    rlgr.SegmentedCoder.encode_ragged(rm, mats, row_major=True)
    for c, m in zip(rm, mats):
        t = rlgr.SegmentedCoder(D, D, 64)
        t.encode(m.t().contiguous())
        assert c.container() == t.container()
    # among channel-major frames: channel-major; among row-major frames: refused unless said
    other = torch.from_numpy(np.rint(rng.laplace(0, 30.0, size=(D, 100))).astype(np.int32)).cuda()
    c100 = rlgr.SegmentedCoder(100, D, 64)
    c100.encode(other)
    mixed = [rlgr.SegmentedCoder(100, D, 64), rlgr.SegmentedCoder(D, D, 64)]
    rlgr.SegmentedCoder.encode_ragged(mixed, [other, mats[0]])
    assert [c.container() for c in mixed] == [c100.container(), alone[0]]
    rows = other.t().contiguous()
    with pytest.raises(ValueError, match="row_major=True"):
        rlgr.SegmentedCoder.encode_ragged(mixed, [rows, mats[0]])
    with pytest.raises(ValueError, match="row_major=True"):
        rlgr.SegmentedCoder.decode_ragged(mixed, outs=[torch.empty_like(rows), torch.empty_like(mats[0])])
    rlgr.SegmentedCoder.encode_ragged(mixed, [rows, mats[0].t().contiguous()], row_major=True)
    assert [c.container() for c in mixed] == [c100.container(), alone[0]]
    o = rlgr.SegmentedCoder.decode_ragged(mixed, outs=[torch.empty_like(rows), torch.empty_like(mats[0])], row_major=True)
    assert torch.equal(o[0], rows) and torch.equal(o[1], mats[0].t())
    with pytest.raises(ValueError):
        rlgr.SegmentedCoder.encode_ragged(mixed, [rows, mats[0]], row_major=False)
