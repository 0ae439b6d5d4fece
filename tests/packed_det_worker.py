"""Run under MIMRL_DETERMINISTIC=1 by tests/test_gpu_packed.py::test_deterministic_build_pads_the_same_bytes (the library is chosen at
import, so the deterministic build gets its own process): mimrl_op_gather_packed of that build against data.Packed.materialize, bit-exact."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from mimrl_amd import _lib                               # noqa: E402
from tests.test_gpu_packed import check_gather_exact    # noqa: E402


def main():
    assert _lib.DETERMINISTIC and _lib.load().mimrl_deterministic() == 1, "not the deterministic build"
    n = check_gather_exact()
    assert _lib.load().mimrl_deterministic() == 1
    print("packed gather exact under the deterministic build:", n, "arrays")


if __name__ == "__main__":
    main()
