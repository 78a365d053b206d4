"""GPU: the plain forward LK kernel (csrc/hip/kernels_lk.hip: lk_plain_kernel over lk_plain.hpp's plain_lk_pair), the cross-check
of the product kernels behind POLYCHASE_LK_VARIANT=1, against the CPU oracle: next_xy, status and err bit for bit, in the
canonical and in the x86 summation order.  Every other GPU test reaches the product kernels; the switch is read once per process,
so the cases run in ONE subprocess (tests/_lk_plain_check.py, which has the scenes and the expected arrays):

  * the six scenes of test_lk_fb_gpu.py (windows 3 .. 31: every LDS sizing of the launch; 1, 2, 3 and 8 targets; targets that lose
    points) and 5 / 13 supplied keypoints at the borders (a partly empty last workgroup).  Both forward outcomes are asserted on
    the oracle per target first -- except for two 'shift' targets (160x120_w15_l2 target 5: 422 of 422 tracked, 160x120_w31_l2
    target 0: 428 of 428), which lose points only in the backward pass and are asserted to be exactly that;
  * the checkerboard, where the two summation orders give different bits (asserted on the oracle first), at windows whose vector
    blocks cover 0 + 7 .. 24 + 7 columns;
  * windows 3, 7, 10, 16 and 31 of tests/lk_subpixel_scene.py: keypoints off the integer grid (w11 == -1 and rounding ties on the
    template side) and out of the frame, the arrays test_lk_subpixel_gpu.py holds the product kernels to;
  * windows 17, 24 and 31 of the checkerboard once more in THIS process, i.e. on the default variant's lk4 kernel, against the same
    expected arrays: the cross-check the plain kernel exists for."""
import os
import subprocess
import sys

import pytest

import _lk_plain_check as check
from polychase_amd import hip

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def plain_lines():
    env = dict(os.environ)
    env.pop("POLYCHASE_ARITH", None)
    env["POLYCHASE_LK_VARIANT"] = "1"
    r = subprocess.run([sys.executable, os.path.join(HERE, "_lk_plain_check.py")], env=env, text=True, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, f"the helper failed:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    return r.stdout.splitlines()


@pytest.mark.parametrize("arith", sorted(check.ARITH))
@pytest.mark.parametrize("case", check.case_names())
def test_plain_kernel_matches_the_oracle(plain_lines, case, arith):
    mine = [l for l in plain_lines if l.split()[1:3] == [case, arith]]
    assert mine == [f"PASS {case} {arith}"], mine


@pytest.mark.parametrize("arith", sorted(check.ARITH))
def test_lk4_matches_the_arrays_the_plain_kernel_matched_above_window_16(arith):
    assert os.environ.get("POLYCHASE_LK_VARIANT", "0") == "0", "this process must run the product kernels"
    ctx = hip.Context(0)
    ctx.set_arithmetic(check.ARITH[arith][0])
    for case in check.LK4_CROSS_CHECKED:
        assert check.board_gpu_mismatch(ctx, case, arith) == "", case
    ctx.close()
