"""Start the ranks of a multi-process test and collect their verdicts.

run_ranks(body, world, *args) starts ``world`` spawn-context processes; each joins one process group and calls
``body(rank, world, *args)`` (a module-level function of the test file). The parent watches the ranks while it waits: a
rank that dies without a word (a segfault, an abort) fails the test at once, and whatever the failure, no rank outlives it --
a launcher that leaves ranks running after one of them has died keeps them on a GPU that others share."""
import os
import queue
import socket
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_POLL = 0.05            # seconds between two looks at the ranks' exit codes while no report arrives


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _cpu_barrier():
    """dist.barrier() asks torch for an accelerator at run time (torch._C._get_accelerator), which initialises HIP and
    opens the GPU in every rank on a machine that has one. CPU-only ranks: an all-reduce of a CPU tensor over gloo
    synchronises them the same way without touching the device."""
    import torch
    import torch.distributed as dist
    dist.all_reduce(torch.zeros(1))


def _entry(rank, world, port, backend, q, body, args):
    """one rank: the repository on sys.path, the process group, the body, the verdict: (rank, "ok", what the body returned)
    or (rank, the traceback, None)"""
    try:
        sys.path.insert(0, ROOT)
        import torch.distributed as dist
        if backend == "nccl":                   # RCCL on the one GPU of the box
            import torch
            torch.cuda.set_device(0)
            dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                                    device_id=torch.device("cuda", 0))
        else:
            os.environ["MASTER_ADDR"] = "127.0.0.1"
            os.environ["MASTER_PORT"] = str(port)
            dist.init_process_group(backend, rank=rank, world_size=world)
        value = body(rank, world, *args)
        dist.destroy_process_group()
        q.put((rank, "ok", value))
    except Exception:
        q.put((rank, traceback.format_exc(), None))


def _stop(procs):
    """terminate every rank still alive; kill the ones that do not leave"""
    live = [p for p in procs if p.is_alive()]
    for p in live:
        p.terminate()
    for p in live:
        p.join(timeout=10)
        if p.is_alive():
            p.kill()
            p.join()


def _others(procs, reported):
    """what is known of the ranks that have not reported, for a failure message"""
    return "; ".join(f"rank {r} " + ("still running" if p.exitcode is None else f"exited with exit code {p.exitcode}, no report")
                     for r, p in enumerate(procs) if r not in reported) or "every other rank reported ok"


def run_ranks(body, world, *args, backend="gloo", report_timeout=420, join_timeout=60):
    """-> what body(rank, world, *args) returned on every rank, in rank order. AssertionError when a rank raises (its
    traceback in the message), exits without reporting (its exit code in the message), lets ``report_timeout`` seconds pass
    without any rank reporting, or is still there ``join_timeout`` seconds after the last report. No rank survives a
    failure, none is restarted, nothing is tried twice."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_entry, args=(r, world, port, backend, q, body, args)) for r in range(world)]
    for p in procs:
        p.start()
    values, suspects = {}, set()
    deadline = time.monotonic() + report_timeout
    try:
        while len(values) < world:
            try:
                rank, verdict, value = q.get(timeout=_POLL)
            except queue.Empty:
                gone = {r for r, p in enumerate(procs) if r not in values and p.exitcode is not None}
                # a rank flushes its report before it exits: one that was gone before the last empty look has sent none
                assert not gone & suspects, f"a rank exited without reporting: {_others(procs, values)}"
                suspects = gone
                assert time.monotonic() < deadline, f"no report for {report_timeout} s ({_others(procs, values)})"
                continue
            assert verdict == "ok", f"rank {rank}:\n{verdict}\n({_others(procs, {rank, *values})})"
            values[rank] = value
            deadline = time.monotonic() + report_timeout
        end = time.monotonic() + join_timeout
        for p in procs:
            p.join(timeout=max(0.0, end - time.monotonic()))
        late = [r for r, p in enumerate(procs) if p.is_alive()]
        assert not late, f"ranks {late} reported ok but did not exit within {join_timeout} s"
    finally:
        _stop(procs)
    return [values[r] for r in range(world)]
