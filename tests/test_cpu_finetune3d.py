"""CPU-side checks of the 3-D fine-tuning loop: the fixture g18_finetune3d itself, the float64 restatement of the loop
(tests/finetune3d_ref.py: the 3-D noise rule around afno3d_ref.model3d_ref) against the reference's records, that the 3-D and
the 2-D noise rules can be told apart at the test tolerance, and the host-side argument checks of the new ops and of the
rollout with a one-output model."""
import os

import pytest
import torch

import afno3d_ref as A3
import finetune3d_ref as F3
from helpers import GOLDEN, assert_sub, load

RTOL = 1e-4


@pytest.fixture(scope="module")
def fx():
    return load("g18_finetune3d")


def _model(tag):
    """this package's DPOTNet3D on the CPU (a parameter container there) with the case's weights, 2-D components loaded"""
    from dpot_amd import DPOTNet3D, load_3d_components_from_2d
    m = DPOTNet3D(**F3.CASES[tag]["cfg"])
    sd3, sd2 = F3.recipe_weights(tag, m)
    m.load_state_dict(sd3)
    load_3d_components_from_2d(m, sd2, ["blocks", "time_agg"])
    return m


def test_fixture_keys_and_size(fx):
    assert os.path.getsize(os.path.join(GOLDEN, "g18_finetune3d.npz")) <= os.path.getsize(os.path.join(GOLDEN, "g17_dpot3d.npz"))
    for tag in F3.CASES:
        names = [str(n) for n in fx[f"{tag}.names"]]
        params = dict(_model(tag).named_parameters())
        assert sorted(names) == sorted(k for k in params if not k.startswith("cls_head."))
        for s in ("loss", "l2_full", "grad_norm"):
            assert f"{tag}.{s}" in fx.files and f"{tag}.err32.{s}" in fx.files
            assert float(fx[f"{tag}.{s}"]) > 0.0
        assert float(fx[f"{tag}.grad_norm"]) > F3.OPT["max_norm"]             # the recorded step was clipped
        for k in (0, 1):
            assert f"{tag}.noisy.{k}.sub" in fx.files and f"{tag}.err32.noisy.{k}" in fx.files
        for n in names:
            assert f"{tag}.g.{n}" in fx.files or f"{tag}.g.{n}.sub" in fx.files, n
            assert f"{tag}.err32.g.{n}" in fx.files and f"{tag}.p.{n}.sub" in fx.files, n
            numel = params[n].numel()
            assert (f"{tag}.g.{n}.sub" in fx.files) == (numel > F3.SUB_MIN), n


@pytest.mark.parametrize("tag", list(F3.CASES))
def test_float64_loop_matches_reference(fx, tag):
    """ties the fixture to a second implementation of model, loss, slide and noise rule"""
    sd = _model(tag).state_dict()
    loss, l2_full, noisy = F3.loop_ref(sd, tag)
    for name, got in (("loss", loss), ("l2_full", l2_full)):
        want = float(fx[f"{tag}.{name}"])
        print(f"{tag}.{name}: float64 loop {got.item():.8f} reference {want:.8f} "
              f"(reference fp32 vs its float64 {float(fx[f'{tag}.err32.{name}']):.2e})")
        assert abs(got.item() - want) <= RTOL * want
    for k in (0, 1):
        assert_sub(noisy[k].float(), fx, f"{tag}.noisy.{k}", f"{tag}.noisy.{k}", rtol=RTOL)


def test_2d_rule_on_the_same_tensor_is_told_apart(fx):
    """the rank-blind reduction (one norm per (b, c) over space and time) misses the recorded noisy input and loss by far
    more than the tolerance the 3-D rule is held to"""
    tag = "ft"
    xx, _, _, eps = F3.inputs(tag)
    a = F3.noise3d(xx.double(), F3.NOISE_SCALE, eps[0].double())
    b = F3.noise2d_rule(xx.double(), F3.NOISE_SCALE, eps[0].double())
    rel = (a - b).abs().max().item() / a.abs().max().item()
    print(f"3-D against 2-D noise rule on the ft input: max|d| / max|a| = {rel:.3e}")
    assert rel > 10 * RTOL
    with pytest.raises(AssertionError):
        assert_sub(b.float(), fx, f"{tag}.noisy.0", "2-D rule", rtol=RTOL)
    loss, _, _ = F3.loop_ref(_model(tag).state_dict(), tag, noise=F3.noise2d_rule)
    want = float(fx[f"{tag}.loss"])
    assert abs(loss.item() - want) > RTOL * want


# ---- host-side checks ----------------------------------------------------------------------------------------------------
def test_ops_refuse_cpu_tensors():
    from dpot_amd import _lib, ops
    x = torch.zeros(1, 4, 4, 4, 2, 1)
    gs, gt = torch.zeros(4), torch.zeros(2)
    with pytest.raises(_lib.DpotHipError):
        ops.patchify3(x, gs, gt, 2)
    with pytest.raises(_lib.DpotHipError):
        ops.unpatchify3(torch.zeros(2 * 8, 5 * 8), 1, 4, 2, 1, 2)
    with pytest.raises(_lib.DpotHipError):
        ops.fold3(torch.zeros(8, 3 * 8), 1, 2, 2, 3)
    with pytest.raises(_lib.DpotHipError):
        ops.fold3(torch.zeros(64, 3), 1, 2, 2, 3, inverse=True)


def test_ops_refuse_a_grid_that_is_no_multiple_of_the_patch():
    from dpot_amd import _lib, ops
    with pytest.raises(_lib.DpotHipError, match="multiple"):
        ops.patchify3(torch.zeros(1, 5, 5, 5, 2, 1), torch.zeros(5), torch.zeros(2), 2)
    with pytest.raises(_lib.DpotHipError, match="multiple"):
        ops.unpatchify3(torch.zeros(16, 40), 1, 5, 2, 1, 2)


def test_noise_dims_rank_rule():
    from dpot_amd import _lib, ops
    assert ops.noise_dims(torch.zeros(2, 4, 5, 3, 2)) == (2, 4 * 5 * 3, 2)              # [B,X,Y,T,C]: per (b, c)
    assert ops.noise_dims(torch.zeros(2, 4, 5, 6, 3, 2)) == (2, 4 * 5 * 6, 3 * 2)       # [B,X,Y,Z,T,C]: per (b, t, c)
    with pytest.raises(_lib.DpotHipError):
        ops.noise_dims(torch.zeros(2, 4, 3, 2))


def test_cls_weight_with_a_one_output_model_raises():
    from dpot_amd import train
    m = _model("ft")
    xx, yy, msk, _ = F3.inputs("ft")
    cls = torch.zeros(F3.B, dtype=torch.int64)
    with pytest.raises(ValueError, match="one tensor"):
        train.rollout_total(m, xx, yy, msk, 1, 0.0, None, cls, 1.0)


def test_rollout_eval_refuses_resize_and_evaluator_for_6d_windows():
    from dpot_amd import infer
    m = _model("ft")
    xx, yy, msk, _ = F3.inputs("ft")
    with pytest.raises(ValueError, match="2-D windows"):
        infer.rollout_eval(m, xx, yy, msk, model_res=8)
    with pytest.raises(ValueError, match="2-D windows"):
        infer.rollout_eval(m, xx, yy, msk, evaluator=object())


def test_new_symbols_in_header_table_and_library():
    import re
    import subprocess
    from dpot_amd import _lib, build
    lib = build.build(verbose=False)
    hdr = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "dpot_hip.h")).read()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    for name in ("dpot_patchify3", "dpot_unpatchify3", "dpot_fold3"):
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", hdr)
        assert m, name
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.c_i, name
        assert args == [_lib.c_i if p.startswith("int ") else _lib.c_fp for p in params], name
        assert f" T {name}\n" in exported, name
    assert _lib.load().dpot_version() >= 269
