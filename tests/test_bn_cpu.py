"""The offset-mean bounds of tests/test_bn_gpu.py hold for the reference alone: BatchNorm with
float64 statistics whose coefficients are then rounded to fp32 the way csrc/bn.hip stores them
(save_mean, save_invstd, scale, shift; the backward's A, B, C), applied with one rounding per fmaf.
Whatever the kernels add to this emulation's error is theirs; the bound is not fitted to them."""
import pytest
import torch

from tests.test_bn_gpu import OFFSET_CASES, offset_case, rel_err

f64 = torch.float64


def _f32(t):
    return t.float().double()


@pytest.mark.parametrize("rows,c", OFFSET_CASES + [(4099, 12)])
@pytest.mark.parametrize("R", [1e3, 3e3])
def test_offset_mean_bounds_hold_for_fp32_coefficients(rows, c, R):
    k = offset_case(rows, c, R)
    y, gamma, beta, dz = k["y"], k["gamma"], k["beta"], k["dz"]
    n = y.shape[0]
    mean, inv = k["mean"], k["inv"]                    # float64 statistics
    mean32, inv32 = _f32(mean), _f32(inv)              # as stored
    scale32, shift32 = _f32(gamma * inv), _f32(beta - mean * gamma * inv)
    z = _f32(y * scale32 + shift32)                    # fmaf: one rounding
    ferr = (z - k["z"]).abs().max().item()
    assert ferr <= k["fwd_bound"], (ferr, k["fwd_bound"])
    # backward: bn_bwd_final's coefficients from the fp32 mean / invstd, sums in float64
    S, Q = dz.sum(0), (dz * (y - mean32)).sum(0)
    dgamma = Q * inv32
    A = gamma * inv32
    B = -gamma * inv32 * inv32 * (dgamma / n)
    C = -A * (S / n) - B * mean32
    A, B, C = _f32(A), _f32(B), _f32(C)
    dy = _f32(A * dz + _f32(B * y + C))
    errs = rel_err(dy, k["dy"]), rel_err(_f32(dgamma), k["dgamma"]), rel_err(_f32(S), k["dbeta"])
    assert max(errs) <= k["bwd_bound"], (errs, k["bwd_bound"])
