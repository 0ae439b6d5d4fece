"""CPU: the --loss menu of the Python surface (MAE, MSE, RMSE, SIMSE, CCC; Solver.py:172-192) -- the flag-to-kind mapping and its
refusals, and the restated losses against the reference's own loss objects (tests/golden/units_losses.npz)."""
import types

import numpy as np
import pytest
import torch

from mimrl_amd import Parameters, Utils, _lib
from tests import task_loss_ref as TL
from tests.helpers import load_golden

LOSSES = ("MAE", "MSE", "RMSE", "SIMSE", "CCC")
UNIT_CASES = (("b2", 2), ("b7", 7), ("b128", 128), ("b1024", 1024), ("const128", 128), ("zero7", 7))   # make_golden_losses.py


def opt(loss):
    return types.SimpleNamespace(loss=loss)


def test_task_loss_code_maps_the_regression_losses():
    assert [_lib.task_loss_code(opt(n)) for n in ("MAE", "MSE", "RMSE", "SIMSE", "CCC")] == [0, 1, 2, 3, 4]
    assert _lib.TASK_LOSSES == TL.KINDS
    assert _lib.task_loss_code(types.SimpleNamespace()) == 0            # an opt without --loss: the reference's default, MAE


@pytest.mark.parametrize("loss", ["Focal", "CE", "BCE"])
def test_task_loss_code_refuses_classification(loss):
    with pytest.raises(NotImplementedError, match="classification"):
        _lib.task_loss_code(opt(loss))


def test_task_loss_code_refuses_unknown():
    with pytest.raises(NotImplementedError, match="unknown"):
        _lib.task_loss_code(opt("Huber"))


def test_task_loss_code_batch_coupled_losses_single_rank_only():
    for loss in ("MAE", "MSE"):
        assert _lib.task_loss_code(opt(loss), world=2) == _lib.TASK_LOSSES[loss]
    for loss in ("RMSE", "SIMSE", "CCC"):
        assert _lib.task_loss_code(opt(loss), world=1) == _lib.TASK_LOSSES[loss]
        with pytest.raises(NotImplementedError, match="couples the whole batch"):
            _lib.task_loss_code(opt(loss), world=2)


def test_header_declares_the_kinds():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = open(os.path.join(root, "include", "mimrl.h")).read()
    found = dict((n, int(v)) for n, v in re.findall(r"MIMRL_TASK_LOSS_([A-Z]+) = (\d+)", h))
    assert found == _lib.TASK_LOSSES


@pytest.mark.parametrize("tag,B", UNIT_CASES)
@pytest.mark.parametrize("name", LOSSES)
def test_restated_losses_equal_the_reference(tag, B, name):
    g = load_golden("units_losses")
    pred, y = g[f"{tag}_pred"], g[f"{tag}_y"]
    assert pred.shape == (B,)
    want_v, want_g = float(g[f"{tag}_{name}_loss"]), g[f"{tag}_{name}_grad"]
    v, grad = TL.value_and_grad(name, pred, y)
    np.testing.assert_allclose(v, want_v, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(grad, want_g, rtol=1e-5, atol=1e-7, equal_nan=True)
    host = Utils.TASK_LOSS_FUNCTIONS[name](torch.from_numpy(pred), torch.from_numpy(y)).item()   # Solver.compute_loss
    np.testing.assert_allclose(host, want_v, rtol=1e-5, atol=1e-7)


def test_fixtures_cover_the_edge_cases():
    g = load_golden("units_losses")
    assert np.all(np.isnan(g["zero7_RMSE_grad"])) and float(g["zero7_RMSE_loss"]) == 0.0   # torch's NaN at a zero residual
    assert np.all(g["zero7_MAE_grad"] == 0.0)
    p = g["const128_pred"]
    assert np.all(p == p[0])                                            # CCC with a zero prediction variance
    assert np.isfinite(g["const128_CCC_grad"]).all()
    assert np.allclose(g["b7_SIMSE_grad"], g["b7_SIMSE_grad"][0])      # the same value in every row


@pytest.mark.parametrize("loss", ["Focal", "CE", "BCE", "RMSE", "MSE", "SIMSE", "MAE", "CCC"])
def test_parameters_accept_every_loss_choice(loss):
    o = Parameters.parse_args(["--loss", loss])
    assert o.loss == loss


@pytest.mark.parametrize("loss", ["MSE", "RMSE", "SIMSE", "CCC"])
def test_solver_accepts_the_regression_losses(loss, monkeypatch):
    """Solver's refusal is task_loss_code now: the four losses pass it (the rest of the constructor needs a GPU)."""
    from mimrl_amd import Solver as S
    calls = []
    monkeypatch.setattr(S._lib, "task_loss_code", lambda o, w=1: calls.append((o.loss, w)) or _lib.TASK_LOSSES[o.loss])
    monkeypatch.setattr(S.mdist, "init_from_env", lambda: (1, 0, 0))
    o = Parameters.parse_args(["--loss", loss, "--optm", "SGD"])
    with pytest.raises(NotImplementedError, match="--optm SGD"):          # past the loss check, stopped by the next one
        S.Solver(o, loaders=())
    assert calls == [(loss, 1)]
