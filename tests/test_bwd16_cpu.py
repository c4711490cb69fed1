"""The fp32-forward / bf16-backward train step (precision "bf16-bwd"), without a device:
construction, the routing plan of its backward conv views, the GPU tests' comparison helpers on
planted errors, and the float emulation the GPU step is compared against
(oracle.emulate_bf16_convs(activations=False, grads=False, ops=("dy", "bx", "bw")))."""
import numpy as np
import pytest
import torch

import tmrnet_amd
from tmrnet_amd import ops
from tests import _bwd16 as H


# ------------------------------------------------------------------ 1. construction
def test_construction_and_keys():
    torch.manual_seed(0)
    m = tmrnet_amd.resnet_lstm(seq_len=2, precision="bf16-bwd")
    f = tmrnet_amd.resnet_lstm(seq_len=2, precision="fp32")
    assert m.share.precision == "bf16-bwd"
    assert list(m.state_dict()) == list(f.state_dict())
    assert all(a.shape == b.shape for a, b in zip(m.state_dict().values(), f.state_dict().values()))
    with pytest.raises(ValueError, match="resnet50 backbone only"):
        tmrnet_amd.resnet_lstm(seq_len=2, precision="bf16-bwd", backbone="resnest50")
    with pytest.raises(ValueError, match="precision must be"):
        tmrnet_amd.resnet_lstm(seq_len=2, precision="fp16")
    with pytest.raises(ValueError, match="precision must be"):
        tmrnet_amd.ResNet50Share(precision="bf16-fwd")


def test_bf16_activations_stay_bf16_only():
    """activations="bf16" keeps requiring precision="bf16" (lfb_build.check_activations)."""
    from tmrnet_amd.lfb_build import check_activations
    m = tmrnet_amd.resnet_lstm(seq_len=2, precision="bf16-bwd")
    check_activations(m, "fp32")
    with pytest.raises(ValueError, match="precision='bf16'"):
        check_activations(m, "bf16")


# ------------------------------------------------------------------ 2. routing plan
# geometries left on the register-staged engine (1), by name -- none
ENGINE1 = ()


@pytest.mark.parametrize("n", [2, 640])
def test_backward_views_plan_lds_dma_or_direct(n):
    """Every ResNet-50 conv's backward views in the step's dtype mix -- dgrad: bf16 dy and bf16
    CRSK weights; wgrad: bf16 x and bf16 dy (the stem: its fp32 NHWC4 input and bf16 dy, the
    direct bf16 stem wgrad; it has no dgrad) -- plan the LDS-DMA engine (2) or a direct kernel
    (0), never the register-staged engine (1)."""
    seen = {}
    for name, h, w, c, k, r, stride, pad in H.resnet50_convs():
        views = [("wgrad", ops.IO_DY if name == "stem" else ops.IO_X | ops.IO_DY)]
        if name != "stem":
            views.append(("dgrad", ops.IO_DY | ops.IO_WT))
        for view, io in views:
            t = ops.conv_tile(n, h, w, c, k, r, r, stride, pad, view, math="bf16", io=io)
            seen[(name, view)] = t["engine"]
            want = (1,) if name in ENGINE1 else (0, 2)
            assert t["engine"] in want, (name, view, t)
    assert seen[("stem", "wgrad")] == 0                    # stem16.hip
    assert seen[("layer1.0.conv2", "wgrad")] == 0          # direct3.hip (bf16 x and dy)
    assert seen[("layer1.0.conv2", "dgrad")] == 2          # fp32 y: not direct3's, the engine
    assert len(seen) == 53 + 52


# ------------------------------------------------------------------ 3. the helpers can fail
@pytest.mark.parametrize("form", ["plain", "res", "apply2"])
def test_compare_apply_catches_planted_errors(form):
    k = H.grid_case(33, 24, 5, form)
    z, bits, z16 = H.emu_apply(k)
    assert (z == 0).sum() >= k["plant"].sum() > 0
    assert H.compare_apply(z, bits, z16, ref_z=z, ref_bits=bits, emu=(z, bits, z16)) == []
    # the last bits word is partial (33 * 24 = 792 = 24 * 32 + 24) and its spare bits are 0
    assert bits.size == 25 and bits[-1] >> 24 == 0
    # (a) a set bit where z == 0
    e = int(np.flatnonzero(z.reshape(-1) == 0)[0])
    wrong = bits.copy()
    wrong[e // 32] |= np.uint32(1 << (e % 32))
    bad = H.compare_apply(z, wrong, z16, ref_z=z, ref_bits=bits)
    assert "bits != fused entry point's bits" in bad and "bits != (z > 0)" in bad
    assert H.compare_apply(z, wrong, z16, emu=(z, bits, z16)) != []
    # (b) truncation instead of RNE in z16
    t16 = H.trunc_bf16(z)
    assert not np.array_equal(t16, z16)          # the case has values that round up
    assert "z16 != RNE(z)" in H.compare_apply(z, bits, t16, ref_z=z, ref_bits=bits)
    # a tie rounds to even, not up: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    ties = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8], dtype=np.float32)
    assert H.rne_bf16(ties).tolist() == [0x3F80, 0x3F82]
    assert np.array_equal(H.rne_bf16(z), torch.from_numpy(z).to(torch.bfloat16)
                          .view(torch.int16).numpy().view(np.uint16))


def test_compare_ds_catches_swapped_outputs():
    g = np.random.default_rng(3)
    dy = g.standard_normal((98, 24)).astype(np.float32)
    dyd = g.standard_normal((98, 24)).astype(np.float32)
    grads = [g.standard_normal(24).astype(np.float32) for _ in range(4)]
    a, b = H.emu_ds_d16(dy, dyd)
    assert H.compare_ds(a, b, grads, dy, dyd, grads) == []
    bad = H.compare_ds(b, a, grads, dy, dyd, grads)            # (c) dy_ds swapped with dy
    assert bad == ["dy != RNE(fp32 dy)", "dy_ds != RNE(fp32 dy_ds)"]
    g2 = [grads[2], grads[3], grads[0], grads[1]]
    assert len(H.compare_ds(a, b, g2, dy, dyd, grads)) == 4
    assert H.compare_ds(H.trunc_bf16(dy), b, grads, dy, dyd, grads) == ["dy != RNE(fp32 dy)"]


# ------------------------------------------------------------------ 4. the emulation step
def test_emulation_step_keeps_the_forward():
    """At 2 frames (B=1, T=2, L=3) the oracle with the three backward roundings gives the fp32
    oracle's logits bit for bit and a different trunk gradient; everything outside the trunk is
    exact (its gradient does not pass through a trunk conv's backward)."""
    r, x, lt, labels, masks = H.step_case()
    e = H.oracle_copy(r, torch.float32, bwd_ops=True)
    f = H.oracle_copy(r, torch.float32)
    out_e, loss_e, ge = H.oracle_step(e, x, lt, labels, masks)
    out_f, loss_f, gf = H.oracle_step(f, x, lt, labels, masks)
    assert torch.equal(out_e, out_f) and torch.equal(loss_e, loss_f)
    for (n, a), (_, b) in zip(e.named_buffers(), f.named_buffers()):
        assert torch.equal(a, b), n
    rel = H.group_rel(ge, gf)
    assert set(rel) == set(H.TRUNK_GROUPS)
    for grp, v in rel.items():
        assert 1e-4 < v < 0.05, (grp, v)       # rounded operands: different, and close
    for n in gf:
        if not n.startswith("share."):
            assert torch.equal(ge[n], gf[n]), n
