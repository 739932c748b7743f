"""Every entry point on a side stream, behind a producer that is still running (include/raht.h: every `stream` argument comes
with a contract -- "enqueues only" or "synchronises `stream`" -- and the Python wrappers pass ``torch.cuda.current_stream()``).

torch's side streams are non-blocking: work that the library puts on the null stream is not ordered against them, and on the default
stream, where the rest of the suite runs, such a slip is invisible. So ``behind_a_delay`` runs a case (tests/stream_cases.py) under
``with torch.cuda.stream(S)`` with its inputs still holding a DECOY when the call is made: a delay kernel of about 50 ms is at the
head of S, the copies that bring the real inputs are queued behind it, and the call comes behind those. A library that reads its
inputs in stream order returns the real answer, bit for bit what it returned on the default stream; one that reads them early, on
another stream or from the host, returns the decoy's answer -- a valid input, so a wrong result and never a fault. No case can pass
vacuously: the decoy's outputs must differ from the real ones, the delay must still be pending when the call is made ("delay too
short" otherwise), and for the entry points the header calls enqueue-only it must still be pending when the call returns. The delay
is a condition of these tests, not a measurement; nothing here is timed but the calibration of the delay itself."""
import ctypes as C
import threading

import numpy as np
import pytest

from . import stream_cases as SC

pytestmark = pytest.mark.gpu

_DELAY = []


def _elapsed_ms(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def delay():
    """enqueue about 50 ms of work on the current stream. Calibrated once per module: a fixed count of ``torch.cuda._sleep`` cycles is
    timed with events and scaled; if that cannot reach 20 ms, a chain of large matmuls is, by the same rule."""
    import torch
    if not _DELAY:
        def sleeper(cycles):
            return lambda: torch.cuda._sleep(cycles)
        _elapsed_ms(sleeper(1000))                                       # (the first launch loads the kernel)
        probe = 1_000_000
        ms = _elapsed_ms(sleeper(probe))
        fn = sleeper(int(probe * 50.0 / ms)) if ms > 1e-3 else None
        if fn is None or _elapsed_ms(fn) < 20.0:
            a = torch.randn(4096, 4096, device="cuda")

            def chain(n):
                def run():
                    b = a
                    for _ in range(n):
                        b = torch.mm(a, b) * 1e-2
                return run
            _elapsed_ms(chain(2))
            fn = chain(max(2, int(16 * 50.0 / max(_elapsed_ms(chain(16)), 1e-3))))
            assert _elapsed_ms(fn) >= 20.0, "no delay of 20 ms can be built on this device"
        _DELAY.append(fn)
    _DELAY[0]()


# ---- comparing nests of outputs -------------------------------------------------------------------------------------------------
def _leaves(x, same=False, out=None):
    """a nest of tensors / arrays / host values -> [(leaf, shared by A and B)], None dropped; a list of host numbers is one leaf"""
    out = [] if out is None else out
    if isinstance(x, SC.Same):
        _leaves(x.value, True, out)
    elif isinstance(x, (list, tuple)) and not all(isinstance(v, (int, float)) for v in x):
        for v in x:
            _leaves(v, same, out)
    elif x is not None:
        out.append((tuple(x) if isinstance(x, (list, tuple)) else x, same))
    return out


def _bytes(t):
    """a tensor's or an array's shape, dtype and bits (``test_gpu_block_modes._bits`` for any element type)"""
    import torch
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous()
        return tuple(t.shape), str(t.dtype), t.reshape(-1).view(torch.uint8).numpy().tobytes()
    if isinstance(t, np.ndarray):
        return t.shape, str(t.dtype), np.ascontiguousarray(t).tobytes()
    return t


def _equal(a, b):
    return _bytes(a) == _bytes(b)


def _clone(x):
    import torch
    if isinstance(x, SC.Same):
        return SC.Same(_clone(x.value))
    if isinstance(x, (list, tuple)):
        return [_clone(v) for v in x]
    return x.clone() if isinstance(x, torch.Tensor) else x


def _assert_is(got, want, what):
    got, want = _leaves(got), _leaves(want)
    assert len(got) == len(want), what
    for n, ((g, _), (w, _)) in enumerate(zip(got, want)):
        assert _equal(g, w), f"{what}: output {n} is not the default-stream result"


def _assert_differ(want, other, what):
    want, other = _leaves(want), _leaves(other)
    assert len(want) == len(other) and any(not s for _, s in want), what
    for n, ((w, same), (o, _)) in enumerate(zip(want, other)):
        assert same or not _equal(w, o), f"{what}: output {n} is the same for the decoy: this case sees nothing, choose other seeds"


def _check_pair(A, B, what):
    import torch
    assert sorted(A) == sorted(B), what
    for k in A:
        assert isinstance(A[k], torch.Tensor) and A[k].is_cuda and A[k].shape == B[k].shape and A[k].dtype == B[k].dtype, (what, k)


# ---- the harness ----------------------------------------------------------------------------------------------------------------
def behind_a_delay(case):
    import torch
    A, B, call = case.build()
    _check_pair(A, B, case.name)
    want, other = _clone(call(A)), _clone(call(B))
    torch.cuda.synchronize()
    _assert_differ(want, other, case.name)
    staging = {k: B[k].clone() for k in B}
    torch.cuda.synchronize()
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        delay()
        for k in staging:
            staging[k].copy_(A[k])
        assert not S.query(), "delay too short: it had finished before the call was made"
        got = call(staging)
        if not case.sync:
            assert not S.query(), f"{case.name}: documented as enqueue-only, but the stream had drained when the call returned"
        got = _clone(got)
    S.synchronize()
    _assert_is(got, want, case.name)
    if case.reads_only:
        for k in staging:
            assert _equal(staging[k], A[k]), f"{case.name}: the call changed its input {k}"
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_on_a_side_stream_behind_a_delayed_producer(name):
    behind_a_delay(SC.CASES[name])


# ---- the rate kernel's host step table ------------------------------------------------------------------------------------------
def test_rate_kernel_has_read_its_host_steps_when_it_returns():
    """raht_rlgr_seg_rate through ctypes (as tests/test_abi_rate.py calls it), behind the delay, with a pageable host step table
    that is overwritten with other valid steps as soon as the call returns, the stream still busy: the sizes are the original steps'"""
    import torch
    from raht_3dgs_codec_amd import _lib
    L = _lib.lib()
    N, D, S_len, k = 5000, 8, 256, 2
    G = D * ((N + S_len - 1) // S_len)
    TA, TB = (SC.dev(SC.attrs(N, D, s) * 40) for s in (1, 2))
    first, second = (0.5, 1.0), (0.25, 3.0)

    def run(T, steps, overwrite=None, stream=None):
        sb = torch.full((k, G), -1, dtype=torch.int32, device="cuda")
        sse = torch.full((k, G), -1.0, dtype=torch.float64, device="cuda")
        st = (C.c_float * k)(*steps)
        rc = L.raht_rlgr_seg_rate(C.c_void_p(T.data_ptr()), _lib.RAHT_F32, D, N, D, st, k, 1, S_len, 1, C.c_void_p(sb.data_ptr()),
                                  C.c_void_p(sse.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if overwrite is not None:
            st[:] = overwrite
            assert not stream.query(), "raht_rlgr_seg_rate is documented as enqueue-only, but the stream had drained when it returned"
        assert rc == 0, L.raht_last_error()
        return [sb, sse]

    want, other, decoy = run(TA, first), run(TA, second), run(TB, first)
    torch.cuda.synchronize()
    _assert_differ(want, other, "steps")
    _assert_differ(want, decoy, "coefficients")
    staging = TB.clone()
    torch.cuda.synchronize()
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        delay()
        staging.copy_(TA)
        assert not S.query(), "delay too short: it had finished before the call was made"
        got = _clone(run(staging, first, overwrite=second, stream=S))
    S.synchronize()
    _assert_is(got, want, "raht_rlgr_seg_rate")


# ---- two streams in turn: the scratch pool's cross-stream rule ------------------------------------------------------------------
def _in_a_thread(fn):
    """the scratch pool is per host thread: a fresh thread starts with an empty one, whatever the tests before this one left"""
    box = []

    def body():
        try:
            fn()
        except BaseException as e:                                       # noqa: BLE001 (re-raised in the test's thread)
            box.append(e)
    t = threading.Thread(target=body)
    t.start()
    t.join()
    if box:
        raise box[0]


def _fill_the_pool():
    """46 calls whose one scratch block (raht_sqdiff_columns: 8 D bytes for one row) each need more than the pool's largest block
    with its 25 % head-room holds: a new block every time, so the thread's pool ends above the 40 blocks from which ``Scratch`` hands
    out a block last used on another stream. The numbers are csrc/device_memory.hip's: a block is bytes + bytes / 4 (growth 1.27 >
    1.25), the pool grows without recycling while it holds fewer than 48 blocks (46 < 48), and `n_dev >= 40` opens the other
    streams' blocks (46 > 40). The library has no counter of the pool's blocks to assert; if those constants change, so must these."""
    import torch
    from raht_3dgs_codec_amd import ops
    D = 2
    for _ in range(46):
        a = torch.zeros((1, D), dtype=torch.float32, device="cuda")
        ops.sqdiff_columns(a, a)
        D = int(np.ceil(D * 1.27)) + 1
    torch.cuda.synchronize()


@pytest.mark.parametrize("pool", ["empty", "above-40-blocks"])
@pytest.mark.parametrize("name", ["mode_search-5", "sort_keys-30-70000", "predict_bi-5"])
def test_two_streams_in_turn(name, pool):
    """A on S1 behind a delay, at once B on S2 with no delay, then A again on S1: three right results -- with a fresh scratch pool,
    and with one large enough to hand S2 a block that S1's call may still be using (csrc/device_memory.hip)"""
    import torch

    def body():
        with torch.cuda.device(0):
            A, B, call = SC.CASES[name].build()
            if pool != "empty":
                _fill_the_pool()
            wantA, wantB = _clone(call(A)), _clone(call(B))
            torch.cuda.synchronize()
            _assert_differ(wantA, wantB, name)
            staging = {k: B[k].clone() for k in B}
            torch.cuda.synchronize()
            S1, S2 = torch.cuda.Stream(), torch.cuda.Stream()
            with torch.cuda.stream(S1):
                delay()
                for k in staging:
                    staging[k].copy_(A[k])
                assert not S1.query(), "delay too short: it had finished before the call was made"
                r1 = call(staging)
                if pool == "empty" and not SC.CASES[name].sync:
                    # S2's call below is made while S1 is still busy (a full pool may wait for the device: that is its rule)
                    assert not S1.query(), f"{name}: documented as enqueue-only, but the stream had drained when the call returned"
                r1 = _clone(r1)
            with torch.cuda.stream(S2):
                r2 = _clone(call(B))
            with torch.cuda.stream(S1):
                r3 = _clone(call(staging))
            S1.synchronize()
            S2.synchronize()
            _assert_is(r1, wantA, f"{name}: first call on S1")
            _assert_is(r2, wantB, f"{name}: call on S2")
            _assert_is(r3, wantA, f"{name}: second call on S1")
            torch.cuda.synchronize()
    _in_a_thread(body)


# ---- a codec path end to end ----------------------------------------------------------------------------------------------------
def test_a_sequence_encodes_and_decodes_on_a_side_stream():
    """I, P, B frames with GPU geometry and GPU entropy, the frames' tensors staged behind the delay: the encode, the full decode and
    a region decode of the I frame (whose top plan takes leaf weights that a kernel has just written) give the default stream's bytes
    and frames. Host synchronisations happen inside: no ``query`` assertion, this shows that the layers compose."""
    import torch
    from raht_3dgs_codec_amd import bitstream
    from .test_gpu_sequence_bidir import J, KW, STEP, _frames
    kw = dict(n_wide=0, gop=3, bframes=1, inter="always", **KW)
    fA, fB = _frames("fade", 5, 3), _frames("fade", 5, 3)
    # the decoy: the scene mirrored through the cube's centre (as many voxels, in Morton order again, none of them A's rows) with
    # other attributes, so that the keys, the octree, the cells' first rows and the leaf weights of the region decode differ too
    fB = [(((1 << J) - 1 - V[::-1]).copy(), (Cm[::-1] * np.float32(1.5)).copy()) for V, Cm in fB]
    assert fB[0][0].shape == fA[0][0].shape and not np.array_equal(fB[0][0], fA[0][0])
    up = lambda fs: [(torch.from_numpy(V).cuda(), torch.from_numpy(Cm).cuda()) for V, Cm in fs]     # noqa: E731
    dA, dB = up(fA), up(fB)
    depth, cells = 2, (0, 8 ** 2 // 2)

    def run(frames):
        blob = bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", **kw)
        dec = bitstream.decode_sequence_bytes(blob, device="cuda")
        V, Cr, _ = bitstream.decode_sequence_region(blob, 0, depth, cells, "cuda")
        return [np.frombuffer(blob, np.uint8), [list(f) for f in dec], V, Cr]

    want, other = _clone(run(dA)), _clone(run(dB))
    torch.cuda.synchronize()
    assert bitstream.sequence_kinds(want[0].tobytes()) == ["I", "B", "P"] and want[2].shape[0] > 0
    _assert_differ(want, other, "sequence")                              # the bytes, every decoded frame's voxels and rows, the region
    staging = [(V.clone(), Cm.clone()) for V, Cm in dB]
    torch.cuda.synchronize()
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        delay()
        for (V, Cm), (VA, CA) in zip(staging, dA):
            V.copy_(VA)
            Cm.copy_(CA)
        assert not S.query(), "delay too short: it had finished before the call was made"
        got = _clone(run(staging))
    S.synchronize()
    _assert_is(got, want, "sequence")
    torch.cuda.synchronize()
