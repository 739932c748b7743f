"""Where the mixed tile kernels fetch their quantization steps, pinned on the gfx950 ISA.

A per-channel step table is indexed by lane, so the compiler reads it from the kernarg segment with vector loads
(`global_load_dword`) and waits for them in front of the first use. tile_body_mx issues those loads at kernel start, next to the
program fetch, and reads a single step as a scalar kernel argument. What this test rules out is the fetch sliding back to where the
steps are used: behind the last barrier of the forward's write-back (all eight waves would sit through a round trip to memory
before the first byte of Q leaves), or behind the barrier at which the inverse's Q rows have landed (the first butterfly round
would wait for it)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raht-3dgs-codec_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """mangled name -> instructions (comments and directives stripped) of every tile_kernel_mx<...> in transform_mx.hip"""
    out = tmp_path_factory.mktemp("isa") / "transform_mx.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-fno-fast-math",
                        "-ffp-contract=on", "-S", "--offload-device-only", os.path.join(CSRC, "transform_mx.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    body, cur = {}, None
    for ln in out.read_text().splitlines():
        m = re.match(r"(_ZN4raht14tile_kernel_mxILb[01]ELb[01]ELi\d+EEEv\w+):", ln)
        if m:
            cur = m.group(1)
            body[cur] = []
            continue
        if cur is None:
            continue
        if ln.startswith(".Lfunc_end"):
            cur = None
            continue
        code = ln.split(";")[0].strip()
        if code and not code.startswith(".") and not code.endswith(":"):
            body[cur].append(code)
    return body


def _kernel(kernels, inv, ident, slots):
    tag = f"tile_kernel_mxILb{int(inv)}ELb{int(ident)}ELi{slots}EE"
    hit = [k for k in kernels if tag in k]
    assert len(hit) == 1, (tag, sorted(kernels))
    return kernels[hit[0]]


def _global_loads(code):
    return [ln for ln in code if ln.startswith("global_load_") and not ln.startswith("global_load_lds_")]


@pytest.mark.parametrize("ident", [True, False])
def test_forward_loads_nothing_behind_its_last_barrier(kernels, ident):
    code = _kernel(kernels, False, ident, 1)
    bars = [i for i, ln in enumerate(code) if ln.startswith("s_barrier")]
    assert len(bars) >= 3, len(bars)
    late = _global_loads(code[bars[-1] + 1:])
    assert not late, late


def test_inverse_loads_nothing_behind_the_barrier_at_which_its_rows_have_landed(kernels):
    code = _kernel(kernels, True, True, 1)
    glds = [i for i, ln in enumerate(code) if ln.startswith("global_load_lds_dwordx4")]
    assert glds, "expected the LDS-direct row loads"
    bars = [i for i, ln in enumerate(code) if ln.startswith("s_barrier") and i > glds[-1]]
    assert bars, "expected a barrier behind the row loads"
    late = _global_loads(code[bars[0] + 1:])
    assert not late, late

