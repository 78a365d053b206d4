"""GPU: who owns what behind the C ABI (DevBuf, PinBuf, Stream, Event of csrc/hip/internal.hpp), seen through
pc_debug_live_resources -- the device allocations, pinned allocations, streams and events the library's objects hold right now.

Every case runs its body (tests/_resource_lifecycle_cases.py) in a fresh child process, so the counts are absolute: they do not
depend on handles other tests still hold or on when Python collects them.

  1. every kind of object alive at once holds something of each of the four kinds, and destroying them in reverse order of
     creation leaves nothing;
  2. a scratch buffer that grows is replaced, not added to;
  3. a creator that refuses returns the code it always returned and holds nothing afterwards -- pc_context_create under a bad
     POLYCHASE_ARITH used to keep four streams and an event per refused call."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NOTHING = [0, 0, 0, 0]
PC_E_INVALID = -1


def _run(case, **env):
    r = subprocess.run([sys.executable, os.path.join(HERE, "_resource_lifecycle_cases.py"), case], env={**os.environ, **env}, text=True,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, f"the child failed:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(case, out)
    return out


def test_everything_alive_holds_each_kind_and_destroying_it_leaves_nothing():
    got = _run("lifecycle")
    assert got["before"] == NOTHING
    assert all(n > 0 for n in got["alive"]), got["alive"]      # a counter that never counts cannot pass
    assert got["after"] == NOTHING


def test_growth_replaces_a_buffer():
    got = _run("growth")
    first, second, third = got["lk_track"]                     # 100, 5000, 100 keypoints
    assert first > 0 and second == first and third == first
    small, large = got["set_keypoints"]                        # 100, 50 000 keypoints on one frame
    assert large == small
    assert got["after"] == NOTHING


def test_context_refused_for_its_arithmetic_keeps_nothing():
    got = _run("bad_arith", POLYCHASE_ARITH="bogus")
    assert got["rc"] == PC_E_INVALID and not got["handle"] and "POLYCHASE_ARITH=bogus" in got["message"]
    assert got["after"] == NOTHING


def test_refusals_hold_nothing():
    got = _run("refusals")
    want = {"frame window 2": "window_size must be in", "analyzer ring 0": "ring_frames must be in", "mesh index": "out of range",
            "refine keypoint": "edge 1 references a keypoint", "pnp from empty set": "is empty"}
    assert [row[0] for row in got["rows"]] == list(want)
    for name, rc, handle, message, before, after in got["rows"]:
        assert rc == PC_E_INVALID and not handle and want[name] in message, (name, rc, message)
        assert after == before, (name, before, after)
    assert got["after"] == NOTHING
