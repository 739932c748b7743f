"""Test-only mixed-precision local ops for raht_3dgs_codec_amd.sharded.ShardedRaht(n_wide > 0): the interface of
sharded.HipLocalOps' mixed calls (forward_quant_mixed / dequant_inverse_mixed with two root buffers, quant_rows_f64 /
dequant_rows_f64) on tests/numpy_ops.NumpyPlan, in float64 on CPU tensors.

Every column is float64 here, so the wide / float split changes no number; what this exercises is the sharded driver's
plumbing: the second buffer set, the second top tree, the split of the top rows' quantization. The float root buffer's
columns [0, n_wide) are UNSPECIFIED in the product (include/raht.h, raht_plan_set_root_buffer_wide): this stand-in fills
them with NaN, so a driver that reads them fails the tests."""
import numpy as np
import torch

from tests.numpy_ops import NumpyLocalOps, _quantize


def _steps(step, D):
    st = torch.as_tensor(step, dtype=torch.float64).reshape(-1)
    if st.numel() not in (1, D):
        raise ValueError("steps must be a scalar or have D entries")
    return st


class NumpyMixedLocalOps(NumpyLocalOps):
    # (the float columns' row quantizers, with per-channel steps as well)
    @staticmethod
    def quant_rows(X, step, pos, Q):
        Q[pos] = _quantize(X.to(torch.float64), _steps(step, X.shape[1]))
        return Q

    @staticmethod
    def dequant_rows(Q, step, pos, out):
        out.copy_((Q[pos].to(torch.float64) * _steps(step, Q.shape[1])).to(out.dtype))
        return out

    @staticmethod
    def quant_rows_f64(X, step, pos, Q):
        assert X.dtype == torch.float64
        Q[pos] = _quantize(X, _steps(step, X.shape[1]))
        return Q

    @staticmethod
    def dequant_rows_f64(Q, step, pos, out):
        assert out.dtype == torch.float64
        out.copy_(Q[pos].to(torch.float64) * _steps(step, Q.shape[1]))
        return out

    @staticmethod
    def forward_quant_mixed(plan, C, step, n_wide, roots=None, roots_wide=None):
        assert (roots is None) == (roots_wide is None)
        assert roots is not None or plan.top_level >= 64, "a truncated plan needs both root buffers"
        T = plan.forward(C.to(torch.float64))
        if roots is not None:
            R = T[plan.root_rows]
            roots_wide.copy_(R[:, :n_wide])
            roots.copy_(R.to(roots.dtype))
            roots[:, :n_wide] = float("nan")                 # unspecified in the product: nobody may read them
        Q = _quantize(T[plan.order_RAGFT], _steps(step, T.shape[1]))
        if roots is not None:
            Q[plan.inv_order[plan.root_rows]] = np.iinfo(np.int32).min      # left to the caller's top stage
        return Q

    @staticmethod
    def dequant_inverse_mixed(plan, Q, step, n_wide, roots=None, roots_wide=None):
        assert (roots is None) == (roots_wide is None)
        assert roots is not None or plan.top_level >= 64, "a truncated plan needs both root buffers"
        T = torch.empty((plan.N, Q.shape[1]), dtype=torch.float64)
        T[plan.order_RAGFT] = Q.to(torch.float64) * _steps(step, Q.shape[1])
        if roots is None:
            return plan.inverse(T)
        R = torch.cat([roots_wide.to(torch.float64), roots[:, n_wide:].to(torch.float64)], dim=1)
        return plan.inverse(T, roots=R)
