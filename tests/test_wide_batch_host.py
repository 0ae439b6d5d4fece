"""CPU tier: the per-rank batch ceiling (MIMRL_MAX_BATCH = 2048, the concat critic MIMRL_MAX_BATCH_CONCAT = 1024) is one named constant of
include/mimrl.h, mirrored by _lib, and mimrl_create refuses a batch above it with an error that names it -- before it touches a device."""
import ctypes as C
import os
import re

import pytest

from mimrl_amd import _lib
from tests.golden.configs import CONFIGS, make_opt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_define(name):
    header = open(os.path.join(ROOT, "include", "mimrl.h")).read()
    m = re.search(r"#define\s+" + name + r"\s+(\d+)", header)
    assert m, name
    return int(m.group(1))


def test_batch_ceiling_constants_match_the_header():
    assert _header_define("MIMRL_MAX_BATCH") == _lib.MAX_BATCH == 2048
    assert _header_define("MIMRL_MAX_BATCH_CONCAT") == _lib.MAX_BATCH_CONCAT == 1024
    assert _header_define("MIMRL_NCE_WS_FLOATS") == _lib.NCE_WS_FLOATS


def _create(critic, batch):
    c = dict(CONFIGS["tiny_sep" if critic == "separate" else "tiny_cat"], B=batch)
    cfg = _lib.make_cfg(make_opt(c), 768, 74, 35, seq_len=c["T"], bank_capacity=4096)
    lib = _lib.load()
    h = C.c_void_p()
    rc = lib.mimrl_create(C.byref(cfg), None, C.byref(h))
    if rc == 0:
        lib.mimrl_destroy(h)
    return rc, lib.mimrl_last_error().decode()


@pytest.mark.parametrize("critic,batch,name", [("separate", 2049, "MIMRL_MAX_BATCH"), ("separate", 4096, "MIMRL_MAX_BATCH"),
                                               ("concat", 1025, "MIMRL_MAX_BATCH_CONCAT"), ("concat", 2048, "MIMRL_MAX_BATCH_CONCAT")])
def test_batch_above_the_ceiling_is_refused_by_name(critic, batch, name):
    rc, msg = _create(critic, batch)
    assert rc == -1, (rc, msg)                                 # MIMRL_ERR_ARG
    assert f"exceeds {name} (" in msg and str(batch) in msg, msg
