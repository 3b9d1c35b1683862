"""CPU: the CKA fixture against a float64 numpy restatement, and the host-side logic of the CKA analysis (checkpoint keys, result layout)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests.helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("n_lt_h", "n_gt_h", "hx_ne_hy", "odd_n5_h100", "offset_1e3", "near_identical", "unrelated")


def np_cka(x, y, debiased=False):
    """Linear CKA in float64 from the centred cross-Gram norms (the quantities the kernels compute)."""
    x = x.astype(np.float64) - x.astype(np.float64).mean(0)
    y = y.astype(np.float64) - y.astype(np.float64).mean(0)
    xy, xx, yy = (np.sum((a.T @ b) ** 2) for a, b in ((x, y), (x, x), (y, y)))
    if not debiased:
        return xy / np.sqrt(xx * yy)
    n = x.shape[0]
    rx, ry = (x * x).sum(1), (y * y).sum(1)

    def deb(t, a, b):
        return t - n / (n - 2.0) * a.dot(b) + a.sum() * b.sum() / ((n - 1) * (n - 2))
    return deb(xy, rx, ry) / np.sqrt(deb(xx, rx, rx) * deb(yy, ry, ry))


def _tool():
    spec = importlib.util.spec_from_file_location("modality_cka_tool", os.path.join(ROOT, "tools", "modality_cka.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", CASES)
def test_numpy_restatement_matches_fixture(name):
    g = load_golden("cka.npz")
    x, y = g[f"case/{name}/x"], g[f"case/{name}/y"]
    assert abs(np_cka(x, y) - float(g[f"case/{name}/cka"])) < 1e-9
    assert abs(np_cka(x, y, True) - float(g[f"case/{name}/cka_debiased"])) < 1e-9


def test_fixture_covers_the_cases():
    g = load_golden("cka.npz")
    shapes = {c: (g[f"case/{c}/x"].shape, g[f"case/{c}/y"].shape) for c in CASES}
    assert any(sx[0] < sx[1] for sx, _ in shapes.values()) and any(sx[0] > sx[1] for sx, _ in shapes.values())
    assert shapes["hx_ne_hy"][0][1] != shapes["hx_ne_hy"][1][1]
    assert shapes["odd_n5_h100"] == ((5, 100), (5, 100))
    assert float(g["case/near_identical/cka"]) > 0.999
    assert float(g["case/unrelated/cka"]) < 0.2
    x = g["case/offset_1e3/x"].astype(np.float64)
    assert np.all(np.abs(x.mean(0)) > 100 * x.std(0))


def test_checkpoint_keys_follow_the_reference_loader():
    tool = _tool()
    w = torch.zeros(2)
    assert tool.checkpoint_state_dict({"state_dict": {"model.gpt_neox.embed_in.weight": w}}) == {"gpt_neox.embed_in.weight": w}
    assert list(tool.checkpoint_state_dict({"model.embed_out.weight": w, "gpt_neox.final_layer_norm.bias": w})) == \
        ["embed_out.weight", "gpt_neox.final_layer_norm.bias"]
    # str.replace drops every "model." in the key, as load_model_from_checkpoint does
    assert list(tool.checkpoint_state_dict({"state_dict": {"model.vision_model.model.x": w}})) == ["vision_x"]


def test_result_keys_and_pickle_layout():
    from mafed_amd.analysis import result_keys
    assert result_keys(3) == ["image:1", "image:2", "image:3", "text:1", "text:2", "text:3"]
    tool = _tool()
    runs = [{"image:1": [0.9, 0.8], "text:1": [0.7, 0.6]}, {"image:1": [0.5, 0.4], "text:1": [0.3, 0.2]}]
    out = tool.stack_runs(runs)
    assert list(out) == ["image:1", "text:1"]
    assert out["image:1"].shape == (2, 2) and out["image:1"].dtype == np.float64
    np.testing.assert_array_equal(out["text:1"], [[0.7, 0.6], [0.3, 0.2]])


def test_modality_cka_rejects_bad_arguments():
    from mafed_amd.analysis import modality_cka
    f = torch.zeros(2, 1, 4, 8)
    with pytest.raises(ValueError):
        modality_cka([f], reference=0)
    with pytest.raises(ValueError):
        modality_cka([f, f], reference=2)
    with pytest.raises(ValueError):
        modality_cka([f, torch.zeros(2, 1, 4, 4)], reference=0)
