"""tests/rank_procs.py itself: a rank that raises fails the test with its traceback; a rank that dies without a word fails
it at once, by its exit code, and takes the ranks it left blocked with it. CPU only."""
import os
import time

import pytest

from tests.rank_procs import run_ranks


def _ranks_return(rank, world, base):
    return base + rank


def _rank_1_raises(rank, world):
    if rank == 1:
        raise ValueError("rank 1 does not like this")
    _blocked_in_a_collective()


def _rank_1_dies(rank, world):
    if rank == 1:
        os._exit(3)                             # no report, no traceback: what a segfault or an abort leaves
    _blocked_in_a_collective()


def _blocked_in_a_collective():
    import torch
    import torch.distributed as dist
    dist.all_reduce(torch.zeros(1))             # the peer never enters it


def _no_rank_left():
    import torch.multiprocessing as mp
    return mp.active_children() == []


def test_bodies_return_in_rank_order():
    assert run_ranks(_ranks_return, 3, 10) == [10, 11, 12]
    assert _no_rank_left()


def test_a_raising_rank_fails_with_its_traceback():
    with pytest.raises(AssertionError, match="rank 1 does not like this") as e:
        run_ranks(_rank_1_raises, 2, report_timeout=120)
    assert "Traceback" in str(e.value) and "_rank_1_raises" in str(e.value)
    assert _no_rank_left()


def test_a_rank_that_dies_silently_fails_at_once_and_takes_its_peers_along():
    """report_timeout is this test's own and the bound on the time well below it, so waiting the timeout out cannot pass: the
    ranks need a few seconds to start (a spawned interpreter importing torch), the launcher a fraction of one to notice."""
    t0 = time.monotonic()
    with pytest.raises(AssertionError, match="exit code 3"):
        run_ranks(_rank_1_dies, 2, report_timeout=120)
    assert time.monotonic() - t0 < 60
    assert _no_rank_left()
