"""The mixed tile kernels (csrc/transform_mx.hip) fetch a per-channel step table at kernel start, next to their tile program, and
read a single step as a scalar argument; what the compiler's own early loads fetched is declared landed behind the wait for the
tile's rows. Aimed at what a wait that comes too early or a wrong step lane would break: waves that issue unequal numbers of row
loads or none, every kind of step table across row widths and wide-channel counts, and repeated calls (a wait that is missing shows
as an intermittent difference).

Every case asserts the identity of tests/test_gpu_mixed.py, forward and inverse: the wide columns are bit for bit what
raht_fwd_quant_f64 / raht_dequant_inv_f64 return, the other columns what raht_fwd_quant / raht_dequant_inv return."""
import pytest

from .test_gpu_mixed import _random_scene

pytestmark = pytest.mark.gpu

SMALL = (64, 64, 0, 64)        # 64-row tiles in every stage: eight waves share at most 15 row-load instructions
AUTO = (0, 0, 0, 0)
NBITS = 30


@pytest.fixture(scope="module")
def rt():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    _lib.lib()
    return R


_scenes = {}


def _scene(rt, N, D):
    """keys and rows of one scene per (N, D), drawn once"""
    if (N, D) not in _scenes:
        keys, C = _random_scene(4000 + N, N, NBITS, D)
        assert C.shape[0] == N
        _scenes[(N, D)] = (keys, C)
    return _scenes[(N, D)]


def _plan(rt, keys, geom, D, nw):
    p = rt.RahtPlan.from_keys(keys, NBITS)
    p.set_engine("tile", *geom)
    assert p.mixed_stats(D, nw)["tile_rows"] >= 64                          # the mixed tile kernels run, not the two-pass path
    return p


def _identity(p, C, steps, nw, tag):
    """forward and inverse against the float64 and float32 kernels; returns the mixed outputs"""
    import torch
    Q = p.forward_quant_mixed(C, steps, nw)
    Q64 = p.forward_quant(C.double(), steps)
    Q32 = p.forward_quant(C, steps)
    assert torch.equal(Q[:, :nw], Q64[:, :nw]), tag
    assert torch.equal(Q[:, nw:], Q32[:, nw:]), tag
    mixq = torch.cat([Q64[:, :nw], Q32[:, nw:]], dim=1).contiguous()
    Cr = p.dequant_inverse_mixed(mixq, steps, nw)
    C64 = p.dequant_inverse(mixq, steps, dtype=torch.float64)
    C32 = p.dequant_inverse(mixq, steps)
    assert torch.equal(Cr[:, :nw], C64[:, :nw].float()), tag
    assert torch.equal(Cr[:, nw:], C32[:, nw:]), tag
    return Q, Cr


@pytest.mark.parametrize("geom,N", [(SMALL, 129), (SMALL, 65), (SMALL, 700), (SMALL, 5000), (AUTO, 1537), (AUTO, 5000)])
def test_waves_with_unequal_numbers_of_row_loads(rt, geom, N):
    """N = 129 in 64-row tiles: the last tile is one row, seven of its waves load nothing; 65: the same with two tiles; 700, 5000:
    partial last tiles, and with 5000 rows several tile stages, so the later-stage and last-stage bodies run; the automatic
    geometry: a partial last tile of the automatic tile height."""
    D, nw = 59, 3
    keys, C = _scene(rt, N, D)
    p = _plan(rt, keys, geom, D, nw)
    if N == 5000:
        stages = p.mixed_stats(D, nw)["rows_per_stage"]
        print(f"N = {N}, geometry {geom}: rows per stage {stages}")
        assert len(stages) >= (2 if geom == SMALL else 1)
    _identity(p, C, 0.013, nw, (geom, N, "scalar"))
    _identity(p, C, [0.01 * (1 + (c % 7)) for c in range(D)], nw, (geom, N, "per channel"))


def _steps(kind, D, nw):
    if kind == "scalar":
        return 0.013
    steps = [0.002 * (3 + c) for c in range(D)]                             # all different
    if kind == "huge":
        steps[nw + (D - nw) // 2] = 2.0 ** 101                              # an attribute channel: no fast division for the table
    return steps


@pytest.mark.parametrize("kind", ["scalar", "distinct", "huge"])
@pytest.mark.parametrize("nw", [1, 3, 4])
@pytest.mark.parametrize("Dsel", ["nw+4", 14, 59, 66])
def test_step_lanes(rt, Dsel, nw, kind):
    """every lane quantizes and dequantizes with the steps of its own channels: a scalar step, a per-channel table with all values
    different, and one whose 2^101 entry sends the whole table down the IEEE-division path (that channel's integers are 0)"""
    D = nw + 4 if Dsel == "nw+4" else Dsel
    N = 700
    keys, C = _scene(rt, N, D)
    p = _plan(rt, keys, SMALL, D, nw)
    steps = _steps(kind, D, nw)
    Q, _ = _identity(p, C, steps, nw, (D, nw, kind))
    if kind == "huge":
        c = nw + (D - nw) // 2
        assert int(Q[:, c].abs().max()) == 0
        assert int(Q[:, nw:].abs().max()) > 0


def test_two_calls_on_one_plan_and_a_repeated_forward(rt):
    """cached tile programs: the second call reads what the first one resolved; ten forwards of one 5000-row scene agree bit for bit"""
    import torch
    D, nw = 59, 3
    keys, C = _scene(rt, 5000, D)
    steps = [0.01 * (1 + (c % 7)) for c in range(D)]
    for geom in (SMALL, AUTO):
        p = _plan(rt, keys, geom, D, nw)
        Q0, C0 = _identity(p, C, steps, nw, (geom, "first call"))
        Q1, C1 = _identity(p, C, steps, nw, (geom, "second call"))
        assert torch.equal(Q0, Q1) and torch.equal(C0, C1)
        for i in range(10):
            assert torch.equal(p.forward_quant_mixed(C, steps, nw), Q0), (geom, i)
            assert torch.equal(p.forward_quant_mixed(C, 0.013, nw), p.forward_quant_mixed(C, 0.013, nw)), (geom, i)
