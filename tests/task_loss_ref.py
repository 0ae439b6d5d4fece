"""The regression task losses of --loss (Solver.py:172-192) restated in fp32 torch for the oracle side of the tests: pinned to the
reference's own loss objects by tests/golden/units_losses.npz (test_task_loss_host.py).  ``patch_oracle`` puts one in the place of the
oracle's MAE (oracle.mimrl_ref.stage_loss looks ``task_loss_mae`` up at call time)."""
import torch

KINDS = {"MAE": 0, "MSE": 1, "RMSE": 2, "SIMSE": 3, "CCC": 4}


def mae(p, y):
    return (p - y).abs().mean()


def mse(p, y):
    return ((p - y) ** 2).mean()


def rmse(p, y):
    return ((p - y) ** 2).mean() ** 0.5


def simse(p, y):
    return (y - p).sum().pow(2) / (p.numel() ** 2)


def ccc(p, y):
    mp, my = p.mean(), y.mean()
    cov = ((p - mp) * (y - my)).mean()
    return 1.0 - 2.0 * cov / (((y - my) ** 2).mean() + ((p - mp) ** 2).mean() + (my - mp) ** 2 + 1e-10)


LOSSES = {"MAE": mae, "MSE": mse, "RMSE": rmse, "SIMSE": simse, "CCC": ccc}


def task_loss(name):
    """The oracle's signature (pred, labels of any shape) -> scalar."""
    fn = LOSSES[name]
    return lambda pred, labels: fn(pred.reshape(-1), labels.reshape(-1))


def value_and_grad(name, pred, y):
    p = torch.as_tensor(pred, dtype=torch.float32).clone().requires_grad_(True)
    loss = LOSSES[name](p, torch.as_tensor(y, dtype=torch.float32))
    loss.backward()
    return loss.item(), p.grad.numpy().copy()


def patch_oracle(monkeypatch, name):
    import oracle.mimrl_ref
    monkeypatch.setattr(oracle.mimrl_ref, "task_loss_mae", task_loss(name))
