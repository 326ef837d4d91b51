"""CPU-side checks of the 3-D fine-tuning path: the float64 restatement tests/afno3d_ref.py (and with it the two transform
definitions the kernels of csrc/dft3.hip implement) against the reference's recorded results, the drop-in state_dict layout
of DPOTNet3D, load_3d_components_from_2d, the host-only support query and the fixture itself."""
import os
import warnings
from collections import OrderedDict

import numpy as np
import pytest
import torch

import afno3d_ref as A3
from helpers import GOLDEN, assert_close, assert_sub, load
from oracle import dpot_ref as R


@pytest.fixture(scope="module")
def fx():
    return load("g17_dpot3d")


@pytest.fixture(scope="module")
def built_lib():
    from dpot_amd import build
    return build.build(verbose=False)


def _cmp(t, fx, key, what):
    if key + ".sub" in fx.files:
        assert_sub(t, fx, key, what)
    else:
        assert_close(t, fx[key], what)


# ---- 1. the restatement against the reference's records ---------------------------------------------------------------
@pytest.mark.parametrize("name", list(A3.AFNO_CASES))
def test_restatement_matches_reference_afno3d(fx, name):
    B, dims, E, nb, modes = A3.AFNO_CASES[name]
    salt = 171 + list(A3.AFNO_CASES).index(name)
    x = R.recipe_input((B, *dims, E), salt).double().requires_grad_(True)
    g = R.recipe_input((B, *dims, E), salt + 50).double()
    ws = [w.double().requires_grad_(True) for w in A3.afno_recipe(E, nb, salt)]
    y = A3.afno3d_ref(x, *ws, nb, modes)
    (y * g).sum().backward()
    for k, t in zip(("y", "dx", "dw1", "db1", "dw2", "db2"), [y, x.grad] + [w.grad for w in ws]):
        _cmp(t.float(), fx, f"afno3d.{name}.{k}", f"afno3d.{name}.{k}")


def test_restatement_matches_reference_block3d(fx):
    c = A3.BLOCK_CASE
    E, nb, mh = c["E"], c["nb"], int(c["E"] * c["mlp_ratio"])
    x = R.recipe_input((c["B"], *c["dims"], E), 175).double().requires_grad_(True)
    g = R.recipe_input((c["B"], *c["dims"], E), 225).double()
    p = OrderedDict((k, v.double().requires_grad_(True)) for k, v in A3.block_recipe(E, nb, mh, 175).items())
    y = A3.block3d_ref(x, p, nb, c["modes"])
    (y * g).sum().backward()
    assert_close(y, fx["block3d.y"], "block3d.y")
    assert_close(x.grad, fx["block3d.dx"], "block3d.dx")
    assert [str(n)[2:] for n in fx["block3d.names"]] == list(p)
    for k, v in p.items():
        assert_close(v.grad, fx[f"block3d.d.{k}"], f"block3d.d.{k}")


def test_irfft3_definition_is_irfftn_of_the_padded_box():
    """the real-part sum with w(kz) is torch.fft.irfftn for a NON-Hermitian spectrum; its adjoint is w * rfftn"""
    gen = torch.Generator().manual_seed(17)
    for dims, m3 in (((4, 4, 4), (4, 4, 3)), ((6, 5, 4), (3, 3, 3)), ((5, 3, 7), (2, 2, 4)), ((4, 3, 16), (2, 2, 8))):
        S = torch.complex(torch.randn(2, *m3, 3, generator=gen, dtype=torch.float64),
                          torch.randn(2, *m3, 3, generator=gen, dtype=torch.float64))
        y = A3.irfft3_def(S, dims, 1)
        assert (y - A3.irfftn_padded(S, dims)).abs().max().item() < 1e-13
        g = torch.randn(2, *dims, 3, generator=gen, dtype=torch.float64)
        for cw in (0, 1):                     # <irfft3_w(S), g> = Re <S, rfft3_w(g)>
            lhs = (A3.irfft3_def(S, dims, cw) * g).sum().item()
            rhs = (S.conj() * A3.rfft3_def(g, m3, cw)).real.sum().item()
            assert abs(lhs - rhs) < 1e-11 * (1 + abs(lhs))
        rows = A3.to_rows(S, 1)
        assert torch.equal(A3.from_rows(rows, 2, m3, 3, 1), S)


# ---- 2. state_dict layout ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,cfg", [("mini", A3.MINI3D), ("mini_norm", A3.MINI3D_NORM),
                                     ("mini_mlp", dict(A3.MINI3D, time_agg="mlp"))])
def test_state_dict_layout_matches_reference(fx, tag, cfg):
    from dpot_amd import DPOTNet3D
    sd = DPOTNet3D(**cfg).state_dict()
    assert list(sd) == [str(k) for k in fx[f"keys.{tag}"]]
    for (k, v), s in zip(sd.items(), fx[f"shapes.{tag}"]):
        assert tuple(v.shape) == tuple(int(d) for d in s[:v.dim()]) and not s[v.dim():].any(), k


def test_constructor_defaults_match_reference():
    import inspect
    from dpot_amd import DPOTNet3D
    sig = inspect.signature(DPOTNet3D.__init__)
    got = [(n, p.default) for n, p in sig.parameters.items() if n != "self"]
    assert got == [("img_size", 224), ("patch_size", 16), ("mixing_type", "afno"), ("in_channels", 1), ("out_channels", 3),
                   ("in_timesteps", 1), ("out_timesteps", 1), ("n_blocks", 4), ("embed_dim", 768), ("out_layer_dim", 32),
                   ("depth", 12), ("modes", 32), ("mlp_ratio", 1.), ("n_cls", 1), ("normalize", False), ("act", "gelu"),
                   ("time_agg", "exp_mlp")]


def test_cpu_input_raises():
    from dpot_amd import DPOTNet3D, _lib
    m = DPOTNet3D(**A3.MINI3D)
    with pytest.raises(_lib.DpotHipError):
        m(torch.zeros(1, 8, 8, 8, 3, 2))


# ---- 3. the loader -------------------------------------------------------------------------------------------------------
def _shapes(m):
    return OrderedDict((k, tuple(v.shape)) for k, v in m.state_dict().items())


def test_load_3d_components_from_2d_matches_reference(fx):
    from dpot_amd import DPOTNet3D, load_3d_components_from_2d
    m = DPOTNet3D(**A3.MINI3D)
    m.load_state_dict(A3.recipe_sd(_shapes(m), A3.MINI3D["n_blocks"], 180))
    src = OrderedDict(("module." + k, v) for k, v in R.recipe_state_dict(R.DPOTConfig(**A3.MINI2D), 181).items())
    ptrs = [p.data_ptr() for p in m.parameters()]
    with pytest.warns(UserWarning, match="no_such_part"):
        load_3d_components_from_2d(m, src, ["blocks", "time_agg", "no_such_part"])
    assert ptrs == [p.data_ptr() for p in m.parameters()]              # copied in place
    sd = m.state_dict()
    sums = np.array([[v.double().sum().item(), v.double().abs().sum().item()] for v in sd.values()])
    assert np.array_equal(sums, fx["loader.sums"])
    assert np.array_equal(torch.cat([v.reshape(-1) for v in sd.values()])[::5].numpy(), fx["loader.sub"])
    # the 2-D channel-MLP weights arrived as Conv3d weights, everything else of the 3-D model kept its values
    assert torch.equal(sd["blocks.1.mlp.0.weight"], src["module.blocks.1.mlp.0.weight"].unsqueeze(-1))
    assert torch.equal(sd["time_agg_layer.w"], src["module.time_agg_layer.w"])
    assert torch.equal(sd["pos_embed"], A3.recipe_sd(_shapes(m), 4, 180)["pos_embed"])


def test_load_3d_unknown_component_changes_nothing():
    from dpot_amd import DPOTNet3D, load_3d_components_from_2d
    m = DPOTNet3D(**A3.MINI3D)
    before = OrderedDict((k, v.clone()) for k, v in m.state_dict().items())
    src = {"model": R.recipe_state_dict(R.DPOTConfig(**A3.MINI2D), 181)}      # a checkpoint dict
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        load_3d_components_from_2d(m, src, ["patch_embed", "out"])           # 2-D names a 3-D model does not take
    assert len(rec) == 2
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k


# ---- 4. the support query (host only) ------------------------------------------------------------------------------------
def test_dft3_supported(built_lib):
    from dpot_amd import ops
    assert ops.dft3_supported((8, 8, 8), 512, ops.kept_modes3((8, 8, 8), 32))
    assert ops.kept_modes3((16, 16, 16), 32) == (16, 16, 8)
    assert ops.dft3_supported((16, 16, 16), 32, (16, 16, 8))
    assert ops.dft3_supported((16, 16, 16), 32, (5, 5, 8))
    assert not ops.dft3_supported((64, 64, 64), 512, ops.kept_modes3((64, 64, 64), 32))
    assert not ops.dft3_supported((40, 40, 40), 32, ops.kept_modes3((40, 40, 40), 32))
    assert ops.dft3_supported((6, 5, 7), 16, ops.kept_modes3((6, 5, 7), 32))
    assert ops.kept_modes3((5, 3, 7), 2) == (2, 2, 4) and ops.kept_modes3((4, 3, 16), 2) == (2, 2, 8)
    assert not ops.dft3_supported((4, 4, 4), 32, (5, 4, 3))                  # kept box outside the grid
    assert not ops.dft3_supported((4, 4, 4), 32, (4, 4, 4))                  # mz > Z/2 + 1


def test_unsupported_model_grid_is_named(built_lib):
    from dpot_amd import DPOTNet3D
    m = DPOTNet3D(img_size=40, patch_size=1, in_channels=1, out_channels=1, embed_dim=8, depth=1, n_blocks=1,
                  out_layer_dim=4)
    with pytest.raises(ValueError, match="40x40x40"):
        m._check_grid()


# ---- 5. the fixture ------------------------------------------------------------------------------------------------------
def test_fixture_contents_and_size(fx):
    path = os.path.join(GOLDEN, "g17_dpot3d.npz")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(GOLDEN, "g4_mini.npz"))
    files = set(fx.files)
    for name in A3.AFNO_CASES:
        for k in ("dw1", "db1", "dw2", "db2"):
            assert f"afno3d.{name}.{k}" in files and f"afno3d.{name}.err32.{k}" in files
        for k in ("y", "dx"):
            assert f"afno3d.{name}.{k}" in files or f"afno3d.{name}.{k}.sub" in files
    assert {"block3d.y", "block3d.dx", "mini.pred", "mini.loss", "mini_norm.pred", "step.loss", "step.grad_norm",
            "loader.sums", "loader.sub"} <= files
    for tag in ("mini", "mini_norm"):
        assert all(str(n).startswith("cls_head.") for n in fx[f"{tag}.nograd"]) and len(fx[f"{tag}.nograd"]) == 6
        assert all(f"{tag}.g.{n}" in files for n in fx[f"{tag}.names"])
    # data only: numbers and name lists
    for k in fx.files:
        assert fx[k].dtype.kind in "fiU", (k, fx[k].dtype)
