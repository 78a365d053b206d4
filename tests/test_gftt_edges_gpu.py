"""GPU: the detection chain at its structural edges -- a value bucket of 512 and of 513 keys (with a detection mask too), four
buckets that fit the sort's LDS buffer only one at a time, candidates at distance exactly min_distance (table kernel and grid
kernel, 64.0 against the next double on one image), a frame of equal responses, 1 / 255 / 256 / 257 candidates, the frame's
border, 4095 / 4096 / 4097 keypoints -- against the CPU oracle: response bits, counts, keypoints in value and order, and the
path the detection took (Context.detection_paths()).  The scenes and their conditions: tests/gftt_dot_scenes.py,
tests/test_gftt_edges_cpu.py; the cases and what a case compares: tests/_gftt_edges_check.py.

Every case runs in this process (the fused chain where the options allow it) and once more in each of two child processes:
POLYCHASE_GFTT_GENERAL=1 (the general chain for the same options) and POLYCHASE_GFTT_SLOW_PATH=1 (every detection redone).

The keypoint buffer: a stage-level frame holds max(4096, w h / 16) * 1.5 + 1024 keypoints (7168 at the least), so 4096 and
4097 keypoints fit it and finish on the fast path with every max_corners (_gftt_edges_check.expected_paths restates the rule;
the path assertions follow it).  Dots at a pitch of 5 px or more cannot reach that capacity in any frame size; the
keypoint_capacity_7167 / 7168 / 7169 scenes (pitch 4, 256 x 256) are the edge itself: 7167 keypoints fit, 7168 are redone for
the keypoint capacity with max_corners 0 and 8000 and stay on the fast path with max_corners 7168 and 5000, and a frame redone
with 7169 has grown its buffer, so its second detection fits."""
import os
import subprocess
import sys

import pytest

import _gftt_edges_check as chk
from polychase_amd import hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name,run", chk.S.cases(), ids=chk.case_names())
def test_edge_scene_matches_oracle_on_the_path_it_was_built_for(ctx, name, run):
    assert chk.mode_of_process() == "default"
    why = chk.run_case(ctx, name, run, "default")
    assert not why, why


def test_expected_paths_of_the_default_process():
    """what the case list asks of detection_paths(), spelled out: only bucket_513 (overflow bit 1) and the keypoint capacity
    scenes leave the fast path"""
    redo_keypoints = {("keypoint_capacity_7168", "max0"): 2, ("keypoint_capacity_7168", "max8000"): 2,     # 7168 fit the buffer as it is
                      ("keypoint_capacity_7169", "max0"): 1, ("keypoint_capacity_7169", "max8000"): 1}     # the redo grows the buffer
    for name, run in chk.S.cases():
        want = chk.expected_paths(name, run, "default", 2)
        assert want["finished"] == 2 and sum(want.values()) == 4, (name, run)
        if name == "bucket_513":
            assert want["redo_overflow_1"] == 2
        else:
            assert want["redo_keypoints"] == redo_keypoints.get((name, run), 0) and want["fast_path"] == 2 - want["redo_keypoints"], (name, run)


@pytest.mark.parametrize("env", ["POLYCHASE_GFTT_GENERAL", "POLYCHASE_GFTT_SLOW_PATH"])
def test_edge_scenes_in_a_child_process(env):
    child_env = {k: v for k, v in os.environ.items() if k not in ("POLYCHASE_GFTT_GENERAL", "POLYCHASE_GFTT_SLOW_PATH")}
    child_env[env] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_gftt_edges_check.py")], env=child_env, cwd=ROOT, text=True,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.split("\n")
    failed = [l for l in lines if l.startswith("FAIL")]
    assert not failed, "\n".join(failed[:20])
    assert [l[5:] for l in lines if l.startswith("PASS ")] == chk.case_names()
