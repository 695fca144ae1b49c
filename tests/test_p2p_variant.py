"""The P2P variant selection (ggrs_amd/csrc/p2p_variant.hpp p2p_choose) is the rule it replaced (no GPU).

tests/check_p2p_variant.cpp holds that rule, the nested launch functions of kernels.hpp before
p2p_choose, and compares the two over ex_game-, brawler- and stub-like games x T in {1, 2, 3, 4,
23, 24, 50} x W in {8, 9} x fan_k in {8, 16} x every boolean launch fact: the flag set, the
dynamic LDS bytes and whether the launch raises its LDS limit must agree, and every chosen flag set
must be one p2p_kernel compiles for (p2p_variant_valid) and one GameOpsT instantiates
(p2p_variant_reachable).  Run for the product and for the RB_SPEC_Q=1 A/B build.
"""
import os
import subprocess

import pytest

_TESTS = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(_TESTS), "ggrs_amd", "csrc")


@pytest.mark.parametrize("spec_q", [0, 1])
def test_p2p_choose_equals_the_nested_rule_it_replaced(tmp_path, spec_q):
    exe = str(tmp_path / "check_p2p_variant")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-DRB_SPEC_Q={spec_q}", "-I", _CSRC, "-o", exe,
                    os.path.join(_TESTS, "check_p2p_variant.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"57344 cases, 0 mismatches (RB_SPEC_Q={spec_q})" in r.stdout  # 4 games x 7 x 2 x 2 x 2^9
