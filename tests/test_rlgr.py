"""RLGR entropy stage. Host code: runs without a GPU.

Golden streams come from the REFERENCE's own coder (python/PyRLGR, built from its sources by
`make -C oracle ref`; tests/golden/gen_golden.py::rlgr_cases). Bar: byte-exact streams, exact
round trips (the reference asserts the same, encode_3dgs.py:242-245)."""
import os
import sys

import numpy as np
import pytest

from .conftest import ROOT, load_golden

G = load_golden("rlgr_streams")
CASES = sorted(k[:-3] for k in G if k.endswith("__x"))


@pytest.fixture(scope="module")
def rl():
    import raht_3dgs_codec_amd as R
    if not os.path.exists(R.SO_PATH):
        R.build()
    from raht_3dgs_codec_amd import rlgr
    return rlgr


@pytest.mark.parametrize("name", CASES)
def test_oracle_restatement_matches_reference_streams(oracle, name):
    x, flag, ref = G[name + "__x"], int(G[name + "__flag"]), G[name + "__bytes"]
    assert np.array_equal(oracle.rlgr_encode(x, flag), ref)
    assert np.array_equal(oracle.rlgr_decode(ref, len(x), flag), x)


@pytest.mark.parametrize("name", CASES)
def test_product_coder_is_byte_exact(rl, name):
    x, flag, ref = G[name + "__x"], int(G[name + "__flag"]), G[name + "__bytes"]
    m = rl.membuf()
    m.rlgrWrite(x, flag)                     # numpy fast path
    m.close()
    assert m.buffer_size() == len(ref) and np.array_equal(m.get_array(), ref)
    m2 = rl.membuf()
    m2.rlgrWrite([int(v) for v in x], flag)  # Python list, as the reference driver passes it
    assert m2.get_buffer() == ref.tolist()
    ns, back = rl.membuf(ref.tolist()).rlgrRead(len(x), flag)
    assert back == x.tolist() and ns >= 0


def test_channels_api_strided_and_threaded(rl, oracle):
    rng = np.random.default_rng(9)
    N, D = 20000, 7
    Q = np.empty((N, D), np.int32)
    for c in range(D):
        Q[:, c] = (rng.laplace(0, 0.3 * 4 ** c, N)).astype(np.int32)
    Q[:, 3] = 0
    streams, _ = rl.encode_channels(Q, 1, nthreads=3)
    for c in range(D):
        assert np.array_equal(streams[c], oracle.rlgr_encode(Q[:, c].astype(np.int64), 1)), c
    back, _ = rl.decode_channels(streams, N, 1, nthreads=2)
    assert np.array_equal(back, Q)
    # padded rows (row stride > D)
    big = np.zeros((N, 12), np.int32)
    big[:, :D] = Q
    s2, _ = rl.encode_channels(big[:, :D], 1, nthreads=1)
    assert all(np.array_equal(a, b) for a, b in zip(streams, s2))


@pytest.mark.parametrize("seed", range(6))
def test_random_round_trips_against_oracle(rl, oracle, seed):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(1, 5000))
    scale = float(10 ** rng.uniform(-1, 5))
    x = np.clip(rng.laplace(0, scale, n), -2 ** 31, 2 ** 31 - 1).astype(np.int64)
    x[rng.random(n) < rng.uniform(0, 0.9)] = 0
    m = rl.membuf()
    m.rlgrWrite(x.astype(np.int32), 1)
    assert np.array_equal(m.get_array(), oracle.rlgr_encode(x, 1))
    _, back = rl.membuf(m.get_array()).rlgrRead(n, 1)
    assert back == x.tolist()


def test_truncated_stream_does_not_crash(rl):
    x = np.arange(-500, 500, dtype=np.int32)
    m = rl.membuf()
    m.rlgrWrite(x, 1)
    buf = m.get_array()[: m.buffer_size() // 2]
    _, back = rl.membuf(buf).rlgrRead(len(x), 1)      # garbage tail, but bounded and no fault
    assert len(back) == len(x)


def _reference_build():
    """The reference's own coder if oracle/_ref/rlgr*.so was built here (`make -C oracle ref`, where its sources are), else None."""
    import importlib
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    if not any(f.startswith("rlgr") for f in (os.listdir(ref_dir) if os.path.isdir(ref_dir) else [])):
        return None
    sys.path.insert(0, ref_dir)
    try:
        ref = importlib.import_module("rlgr")
    except Exception:
        return None
    finally:
        sys.path.remove(ref_dir)
    return ref if hasattr(ref, "membuf") else None


# the reference coder's streams for the inputs of tests/rlgr_inputs.py, as lengths and SHA-256 digests
# (tests/golden/gen_golden.py::rlgr_random_cases)
RANDOM = load_golden("rlgr_random")


def test_reference_build_agrees_when_present(rl):
    """A 30 000-symbol Laplacian stream: byte-identical to what the reference's coder wrote for it (stored digest), and live
    against its build when that is present."""
    from .rlgr_inputs import digest, laplace_stream
    x = laplace_stream()
    assert np.array_equal(digest(x), RANDOM["lap_x_sha256"]), "seeded input differs from the one the digests were made for"
    b = rl.membuf(); b.rlgrWrite(x, 1)
    got = np.frombuffer(bytes(b.get_buffer()), dtype=np.uint8)
    assert len(got) == int(RANDOM["lap_len"]) and np.array_equal(digest(got), RANDOM["lap_sha256"])
    ref = _reference_build()
    if ref is not None:
        a = ref.membuf(); a.rlgrWrite(x.tolist(), 1); a.close()
        assert a.get_buffer() == b.get_buffer()


def test_random_streams_round_trip_and_match_the_reference_build_when_present():
    """300 random sequences (all-zero, sparse, dense, full int32 range, rare large values, wide normals) and one very long
    run: exact round trip; the 300 byte-identical to what the reference's own coder wrote for them (stored digests), and live
    against its build when that is present (oracle/_ref, built by `make -C oracle ref` where its sources are)."""
    from raht_3dgs_codec_amd import rlgr
    from .rlgr_inputs import digest, random_sequences
    ref = _reference_build()
    xs = random_sequences()
    assert len(xs) == 300 and np.array_equal(RANDOM["x_len"], [len(x) for x in xs])
    assert np.array_equal(np.stack([digest(x) for x in xs]), RANDOM["x_sha256"]), "seeded inputs differ from the digested ones"
    cases = list(zip(xs, RANDOM["bytes_len"], RANDOM["sha256"]))
    cases.append((np.zeros(300_000, dtype=np.int32), None, None))   # one very long run: the run parameter keeps growing
    checked = 0
    for x, n_bytes, sha in cases:
        streams, _ = rlgr.encode_channels(x.reshape(1, -1), 1, nthreads=1, channel_major=True)
        back, _ = rlgr.decode_channels(streams, x.shape[0], 1, nthreads=1, channel_major=True)
        assert np.array_equal(back.reshape(-1), x)
        if sha is not None:
            s = np.frombuffer(streams[0].tobytes(), dtype=np.uint8)
            assert len(s) == int(n_bytes) and np.array_equal(digest(s), sha)
            checked += 1
        if ref is not None and x.shape[0] <= 3000:
            m = ref.membuf()
            m.rlgrWrite(x.tolist(), 1)
            m.close()
            assert bytes(bytearray(m.get_buffer())) == streams[0].tobytes()
    assert checked == 300


# the reference coder's streams for tests/rlgr_inputs.extreme_sequences (tests/golden/gen_golden.py::rlgr_extreme_cases)
EXTREME = load_golden("rlgr_extreme")


def test_the_limits_of_int32_match_the_reference_coder(rl, oracle):
    """INT32_MIN and INT32_MAX -- what a saturated quantizer writes (include/raht.h) -- in runs of 1, 2, 63, 64 and 65, alternating,
    isolated in a zero run, first and last: the host coder's streams are the reference coder's (stored lengths and digests; its
    build, where present, is asked too), and they decode to the input. The reference coder read every one of its own streams back
    to the input when the fixture was made (``round_trips`` all true), so no sequence is pinned to the product alone."""
    from .rlgr_inputs import digest, extreme_sequences
    seqs = extreme_sequences()
    assert [n for n, _ in seqs] == EXTREME["names"].tolist()
    assert np.array_equal(np.stack([digest(x) for _, x in seqs]), EXTREME["x_sha256"]), "inputs differ from the digested ones"
    assert EXTREME["round_trips"].all()
    ref = _reference_build()
    for i, (name, x) in enumerate(seqs):
        assert (x == -2 ** 31).any() or (x == 2 ** 31 - 1).any(), name
        m = rl.membuf()
        m.rlgrWrite(x, 1)
        got = m.get_array()
        assert len(got) == int(EXTREME["bytes_len"][i]) and np.array_equal(digest(got), EXTREME["sha256"][i]), name
        assert np.array_equal(got, oracle.rlgr_encode(x.astype(np.int64), 1)), name
        _, back = rl.membuf(got).rlgrRead(len(x), 1)
        assert back == x.tolist(), name
        assert np.array_equal(oracle.rlgr_decode(got, len(x), 1), x), name
        streams, _ = rl.encode_channels(x.reshape(1, -1), 1, nthreads=1, channel_major=True)
        assert streams[0].tobytes() == got.tobytes(), name
        back2, _ = rl.decode_channels(streams, len(x), 1, nthreads=1, channel_major=True)
        assert np.array_equal(back2.reshape(-1), x), name
        if ref is not None:
            a = ref.membuf(); a.rlgrWrite(x.tolist(), 1); a.close()
            assert bytes(bytearray(a.get_buffer())) == got.tobytes(), name


def test_channel_coder_keeps_one_arena_and_checks_round_trips():
    """ChannelCoder (the pipeline's glue-free path): same bytes as encode_channels, decode into a caller's array, threaded
    equality with the position of the first difference."""
    from raht_3dgs_codec_amd import rlgr
    rng = np.random.default_rng(5)
    N, D = 50000, 7
    Q = np.rint(rng.laplace(0, 3.0, size=(D, N))).astype(np.int32)
    Q[3] = 0
    cc = rlgr.ChannelCoder(N, D, 1, nthreads=3)
    for rep in range(2):                                      # the arena is reused
        cc.encode(Q)
        ref, _ = rlgr.encode_channels(Q, 1, nthreads=2, channel_major=True)
        assert [bytes(s) for s in cc.streams()] == [bytes(s) for s in ref]
        assert cc.size_bytes == sum(len(s) for s in ref)
        out = np.empty_like(Q)
        cc.decode(out)
        assert rlgr.arrays_equal(out, Q, 4)
        if rep == 0:
            Q = Q[:, ::-1].copy()
    out[5, 1234] += 1
    assert not rlgr.arrays_equal(out, Q, 4)
    import ctypes as C
    from raht_3dgs_codec_amd import _lib
    first = C.c_int64()
    _lib.check(_lib.lib().raht_i32_equal(out.ctypes.data_as(C.c_void_p), Q.ctypes.data_as(C.c_void_p), out.size, 3, C.byref(first)))
    assert first.value == 5 * N + 1234
