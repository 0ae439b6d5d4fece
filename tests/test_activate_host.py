"""CPU tier: --activate elu | leakyrelu | hardtanh.  make_cfg stores the MIMRL_ACT_* code of include/mimrl.h, the reference's three other
choices (prelu, rrelu, hardshrink: Utils.py:84-97) are refused by name with the reason, validate_cfg (host code) refuses an activation code
outside the enum instead of training with the identity, and the oracle's activation table -- what tests/test_gpu_activate.py judges the
kernels against -- is torch.nn's modules with their default arguments, bit for bit."""
import ctypes as C
import os
import re

import pytest
import torch

from mimrl_amd import _lib
from oracle import mimrl_ref as R
from tests.golden.configs import CONFIGS, make_opt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"elu": "MIMRL_ACT_ELU", "leakyrelu": "MIMRL_ACT_LEAKYRELU", "hardtanh": "MIMRL_ACT_HARDTANH"}
OLD = {"none": "MIMRL_ACT_NONE", "relu": "MIMRL_ACT_RELU", "gelu": "MIMRL_ACT_GELU", "tanh": "MIMRL_ACT_TANH"}


def _header_enum(name):
    header = open(os.path.join(ROOT, "include", "mimrl.h")).read()
    m = re.search(r"\b" + name + r"\s*=\s*(\d+)", header)
    assert m, name
    return int(m.group(1))


def _cfg(activate="gelu"):
    c = CONFIGS["tiny_sep"]
    opt = make_opt(c)
    opt.activate = activate
    return _lib.make_cfg(opt, 768, 74, 35, seq_len=c["T"], bank_capacity=c["N"])


@pytest.mark.parametrize("name", list(NEW))
def test_make_cfg_accepts_the_new_activations(name):
    assert _cfg(name).activation == _header_enum(NEW[name]) == _lib.ACTS[name]
    assert (_header_enum("MIMRL_ACT_ELU"), _header_enum("MIMRL_ACT_LEAKYRELU"), _header_enum("MIMRL_ACT_HARDTANH")) == (4, 5, 6)


@pytest.mark.parametrize("name", list(OLD))
def test_existing_activation_codes_did_not_move(name):
    assert _lib.ACTS[name] == _header_enum(OLD[name]) == list(OLD).index(name)


@pytest.mark.parametrize("name,why", [("prelu", "learnable"), ("rrelu", "random"), ("hardshrink", "oracle")])
def test_the_other_reference_activations_are_refused_by_name(name, why):
    with pytest.raises(_lib.MimrlError) as e:
        _cfg(name)
    assert f"--activate {name}" in str(e.value) and why in str(e.value), str(e.value)


def test_an_unknown_name_is_refused_too():
    with pytest.raises(_lib.MimrlError) as e:
        _cfg("swish")
    assert "--activate swish" in str(e.value)


@pytest.mark.parametrize("code", [7, -1, 255])
def test_layout_refuses_an_activation_code_outside_the_enum(code):
    lib = _lib.load()
    cfg = _cfg("gelu")
    assert lib.mimrl_layout_count(C.byref(cfg)) > 0
    cfg.activation = code
    rc = lib.mimrl_layout_count(C.byref(cfg))
    msg = lib.mimrl_last_error().decode()
    assert rc == -1, (rc, msg)                                   # MIMRL_ERR_ARG
    assert "activation" in msg and str(code) in msg and "MIMRL_ACT_HARDTANH" in msg, msg


@pytest.mark.parametrize("code", range(0, 7))
def test_layout_accepts_every_activation_code_of_the_enum(code):
    cfg = _cfg("gelu")
    cfg.activation = code
    assert _lib.load().mimrl_layout_count(C.byref(cfg)) > 0


@pytest.mark.parametrize("name,module", [("gelu", torch.nn.GELU), ("relu", torch.nn.ReLU), ("tanh", torch.nn.Tanh), ("elu", torch.nn.ELU),
                                         ("leakyrelu", torch.nn.LeakyReLU), ("hardtanh", torch.nn.Hardtanh)])
def test_oracle_activation_table_is_torch_nn_with_default_arguments(name, module):
    """Values AND derivatives, on a float64 grid that contains the seams -1, 0 and 1 exactly."""
    grid = torch.cat([torch.linspace(-4, 4, 1601, dtype=torch.float64), torch.tensor([-1.0, 0.0, 1.0], dtype=torch.float64)])
    assert all((grid == s).any() for s in (-1.0, 0.0, 1.0))
    a, b = grid.clone().requires_grad_(True), grid.clone().requires_grad_(True)
    ya, yb = R._act(name)(a), module()(b)
    assert torch.equal(ya, yb)
    ga, gb = torch.autograd.grad(ya.sum(), a)[0], torch.autograd.grad(yb.sum(), b)[0]
    assert torch.equal(ga, gb)
