"""The model of an RLGR decoder on damaged bytes (tests/numpy_rlgr_damaged.py) against the decoders that exist on the host: the
oracle's restatement of the reference loop, the host coder's rlgrRead, and the reference's own build where oracle/_ref holds it.
Runs without a GPU. The GPU decoders are held to the same model, on the same cases, by tests/test_gpu_rlgr_damaged.py."""
import numpy as np
import pytest

from . import numpy_rlgr_damaged as M
from . import rlgr_damage_cases as DC
from .test_rlgr import _reference_build

SEEDS = (0, 1, 2, 3)                                                     # (the GPU test applies seed 0)


@pytest.fixture(scope="module")
def rl():
    import os
    import raht_3dgs_codec_amd as R
    if not os.path.exists(R.SO_PATH):
        R.build()
    from raht_3dgs_codec_amd import rlgr
    return rlgr


@pytest.fixture(scope="module")
def all_cases(rl):
    """-> [(frame, seed, name, g, n symbols, clean symbols, bytes a decoder sees)] over every frame and seed"""
    out = []
    for fname, N, D, S in DC.SHAPES:
        _, _, _, Q = DC.frame(fname)
        segs = DC.host_segments(Q, S)
        blob, offs, lens = DC.container(segs)
        nseg = (N + S - 1) // S
        for seed in SEEDS:
            for name, g, damage in DC.build(segs, seed, DC.fragile_segments(fname, N, D, S)):
                c, s = divmod(g, nseg)
                out.append((fname, seed, name, g, DC.symbols_of(N, S, g), Q[c, s * S: (s + 1) * S].astype(np.int64),
                            DC.seen_bytes(blob, offs, lens, g, damage)))
    return out


def test_the_builder_makes_every_kind_for_every_frame(all_cases):
    kinds = ({f"cut_table_{k}" for k in DC.CUTS} | {f"cut_zeros_{k}" for k in DC.CUTS}
             | {"flip_first", "flip_last", "flip_random", "random_bytes", "all_zero", "neighbour", "longer", "sat_all_ff", "sat_zeros_then_ff"})
    for fname, _, _, _ in DC.SHAPES:
        for seed in SEEDS:
            got = {c[2] for c in all_cases if c[0] == fname and c[1] == seed}
            assert kinds <= got, (fname, seed, sorted(kinds - got))
        assert any(c[4] == 1 for c in all_cases if c[0] == fname) or fname == "wide"      # the last segment of one symbol is dealt
    assert any("_fragile" in c[2] for c in all_cases if c[0] == "noise")
    a, b = (DC.build(DC.host_segments(DC.frame("pieces")[3], 1024), 0) for _ in range(2))
    assert a == b                                                                        # seeded: the CPU and the GPU test see the same cases


def test_clean_segments_decode_to_the_frame(all_cases, rl):
    """the model is a decoder: clean streams give the symbols that were coded, inside the domain, with no run past the end"""
    for fname, N, D, S in DC.SHAPES:
        Q = DC.frame(fname)[3]
        segs = DC.host_segments(Q, S)
        nseg = (N + S - 1) // S
        for g in range(0, len(segs), max(1, len(segs) // 9)):
            c, s = divmod(g, nseg)
            seq, info = M.decode(segs[g], DC.symbols_of(N, S, g))
            assert seq == Q[c, s * S: (s + 1) * S].tolist() and not info["left_domain"] and not info["overshoot"], (fname, g)
            assert info["bits"] <= 8 * len(segs[g]) and 8 * len(segs[g]) - info["bits"] < 8, (fname, g)   # (all of it, but the padding)


def test_no_bits_decode_to_the_pattern_worked_out_by_hand():
    assert M.empty_stream_pattern(10) == [0, 0, -1, -1, -1, 0, -1, -1, -1, 0]
    for n in (1, 2, 3, 63, 64, 65, 200, 1024):
        for buf in (b"", bytes(1), bytes(7), bytes(4 * n)):
            seq, info = M.decode(buf, n)
            assert seq == M.empty_stream_pattern(n) and not info["left_domain"], (n, len(buf))


def test_the_model_is_the_oracle_the_host_coder_and_the_reference_build_inside_its_domain(all_cases, oracle, rl):
    """Every in-domain case: the model's symbols are those of oracle.rlgr_decode and of the host coder's rlgrRead on the same bytes
    followed by zeros (32 n + 64 of them: no symbol takes more than 13 bytes, and the oracle's reader -- like the reference's --
    underflows at the end of its buffer and must never get there), and those of the reference's own build where it is present and
    the model says that no run reaches past symbol n (the reference's loop writes past its output there).
    The cap: at most 2 % of the in-domain cases may leave the model's domain and be left out. The kinds were chosen to stay inside;
    the share is asserted, not reported."""
    ref = _reference_build()
    in_domain = [c for c in all_cases if not DC.is_saturating(c[2])]
    assert len(in_domain) >= 250
    left_out, asked_ref = [], 0
    for fname, seed, name, g, n, clean, seen in in_domain:
        seq, info = M.decode(seen, n)
        assert len(seq) == n
        if info["left_domain"]:
            left_out.append((fname, seed, name, g))
            continue
        what = (fname, seed, name, g)
        padded = np.concatenate([np.frombuffer(seen, np.uint8), np.zeros(32 * n + 64, np.uint8)])
        assert oracle.rlgr_decode(padded, n, 1).tolist() == seq, what
        _, host = rl.membuf(padded).rlgrRead(n, 1)
        assert host == seq, what
        if ref is not None and not info["overshoot"]:
            _, theirs = ref.membuf(padded.tolist()).rlgrRead(n, 1)
            assert list(theirs) == seq, what
            asked_ref += 1
        if name == "longer":
            assert seq == clean.tolist(), what                        # (a decoder stops at symbol n, wherever the table says the bytes end)
        if name == "all_zero" or name == "cut_table_0":
            assert seq == M.empty_stream_pattern(n), what
        if name.startswith("cut_zeros_"):                             # zeroing the tail and cutting there are one stream
            cut = DC._cut_at(name.split("_")[2], len(seen))
            assert M.decode(seen[:cut], n)[0] == seq, what
    share = len(left_out) / len(in_domain)
    assert share <= 0.02, (f"{len(left_out)} of {len(in_domain)} in-domain cases left the model's domain ({100 * share:.2f} %; the cap is 2 %, "
                           f"and the fixed seeds gave 0 of 360 = 0.00 % when this test was written): {left_out}")
    assert ref is None or asked_ref >= len(in_domain) // 2
    print(f"[rlgr_damaged] {len(left_out)} of {len(in_domain)} in-domain cases left the domain ({100 * share:.2f} %); "
          f"reference build asked for {asked_ref}")


def test_the_saturating_kinds_do_leave_the_domain(all_cases):
    """... most of them: what they are for. (A segment of a few symbols ends before its state can overflow.)"""
    sat = [c for c in all_cases if DC.is_saturating(c[2])]
    left = sum(M.decode(seen, n)[1]["left_domain"] for _, _, _, _, n, _, seen in sat)
    assert sat and left >= len(sat) // 3, (left, len(sat))
