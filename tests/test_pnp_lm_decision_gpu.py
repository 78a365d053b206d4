"""GPU: the DECISION step of the device-resident Levenberg-Marquardt solver (csrc/hip/pnp_lm.hpp) on scripted sums, through
pc_debug_lm_decide: the wavefront version the tracker runs by default (mode 0), its one-lane cross-check (mode 1) and the bare
one-lane decision of pc_pnp_solve (mode 2) -- against each other and against the numpy restatement of the reference's loop
(tests/pnp_lm_ref.py), over the scripts of tests/pnp_lm_scripts.py, which reach the branches no scene of the suite reaches (failed
pivots, lambda at its limits, the tolerance exits, rho <= 0, the intrinsics bounds, a zero rotation, non-finite sums, the
tracker's correspondence-count rules and its round limit).  Three launches in all.

What is compared how:
  * every integer and every float32 that does not pass through sinf / cosf: bit for bit (a NaN against a NaN);
  * the quaternions of cam / cam_new and the sweep's R -- the only values behind the device's sinf / cosf, which are not numpy's:
    within 4 x the float32-vs-float64 noise the restatement measures on its finite, well-conditioned scripts
    (profiles/pnp_lm_quaternion_noise.txt; test_pnp_lm_ref_cpu.py).  4: an ocml sinf / cosf a couple of ulp looser than numpy's; a
    wrong lane or a swapped term moves a component by parts in a thousand.  Against the float64 shadow on those scripts; against
    the float32 restatement on ALL scripts -- on an ill-conditioned script float32 and float64 are different trajectories (their
    steps are rotations by up to 1e8 rad and the quaternions differ by up to 2), but the device's step is the restatement's bit
    for bit there too, so its quaternion is the restatement's up to sinf / cosf.  The scripted sums do not depend on the camera:
    the tolerance cannot leak into the control flow."""

import numpy as np
import pytest

import pnp_lm_ref as ref
import pnp_lm_scripts as S
from polychase_amd import hip

pytestmark = pytest.mark.gpu

INT_FIELDS = ("convention_opencv", "sweep_optimize_focal", "sweep_optimize_pp", "iterations", "invalid_steps", "rebuild", "phase", "done",
              "n_valid", "status", "optimize_focal", "optimize_pp")
EXACT_FIELDS = ("JtJ", "diag", "Jtr", "step", "cost", "initial_cost", "lambda", "v", "grad_norm", "step_norm", "t", "fx", "fy", "cx", "cy",
                "aspect_ratio")
CAMERA_EXACT = ("t", "fx", "fy", "cx", "cy", "aspect_ratio", "convention_opencv")
MODES = {"wave": hip.LM_DECIDE_WAVE, "serial": hip.LM_DECIDE_SERIAL, "bare": hip.LM_DECIDE_BARE}


def pack(scripts):
    options = np.zeros(len(scripts), hip.PNP_SOLVE_OPTIONS_DTYPE)
    cameras = np.zeros(len(scripts), hip.PNP_CAMERA_DTYPE)
    for k, s in enumerate(scripts):
        for name, v in dict(ref.OPTION_DEFAULTS, **s["options"], rounds_hint=s["max_rounds"]).items():
            options[name][k] = v
        for name, v in dict(ref.CAMERA_DEFAULTS, **s["camera"]).items():
            cameras[name][k] = v
    return options, cameras, np.stack([s["sums"] for s in scripts])


@pytest.fixture(scope="module")
def device():
    """{mode name: states [scripts][rounds]}: one launch per mode over the whole script set"""
    ctx = hip.Context(0)
    options, cameras, sums = pack(S.all_scripts())
    out = {name: ctx.lm_decide(mode, options, cameras, sums) for name, mode in MODES.items()}
    ctx.close()
    return out


@pytest.fixture(scope="module")
def restated():
    return {"wave": S.reference_runs(ref.SERIAL), "serial": S.reference_runs(ref.SERIAL), "bare": S.reference_runs(ref.BARE)}


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    """elementwise: the same 32 bits, or a NaN on both sides"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    if a.dtype != np.float32:
        return a == b
    return (words(a) == words(b)) | (np.isnan(a) & np.isnan(b))


def same_records(a, b):
    """records of LM_DEBUG_STATE_DTYPE -> per record: every word the same, or a float NaN on both sides"""
    ok = np.ones(a.shape, bool)
    for name in a.dtype.names:
        if a.dtype[name].names:
            ok &= same_records(a[name], b[name])
        else:
            ok &= same_bits(a[name], b[name]).reshape(a.shape + (-1,)).all(axis=-1)
    return ok


def report(scripts, bad, what):
    where = np.argwhere(bad)
    names = sorted({scripts[i]["name"] for i in where[:, 0]})
    return f"{what}: {len(where)} snapshots of {len(names)} scripts differ, first {where[0].tolist()}; scripts {names[:12]}"


def test_wave_decision_is_the_serial_decision_bit_for_bit(device):
    scripts = S.all_scripts()
    bad = ~same_records(device["wave"], device["serial"])
    assert not bad.any(), report(scripts, bad, "wave vs serial")
    # the bare decision is the tracker's where no tracker rule applies (n_valid, which only the tracker's rules set, left out)
    free = np.array([s["max_rounds"] == 0 and bool((s["sums"][:, 54] >= 4).all()) for s in scripts])
    assert free.sum() >= 400
    a, b = device["bare"][free].copy(), device["serial"][free].copy()
    a["n_valid"] = b["n_valid"] = 0
    bad = ~same_records(a, b)
    assert not bad.any(), report([s for s, f in zip(scripts, free) if f], bad, "bare vs serial")


@pytest.mark.parametrize("mode", list(MODES))
def test_device_decision_is_the_restatement(device, restated, mode):
    scripts = S.all_scripts()
    got = device[mode]
    want = np.stack([r.states for r in restated[mode]])
    for name in INT_FIELDS:
        bad = got[name] != want[name]
        assert not bad.any(), report(scripts, bad, name)
    for name in EXACT_FIELDS:   # (JtJ: all 81 entries -- the upper triangle stays zero, as in the restatement)
        bad = ~same_bits(got[name], want[name]).reshape(got.shape + (-1,)).all(axis=-1)
        assert not bad.any(), report(scripts, bad, name)
    upper = np.triu_indices(9, 1)
    assert not got["JtJ"].reshape(got.shape + (9, 9))[..., upper[0], upper[1]].view(np.uint32).any(), "JtJ's upper triangle is written"
    for cam in ("cam", "cam_new"):
        for name in CAMERA_EXACT:
            bad = ~same_bits(got[cam][name], want[cam][name]).reshape(got.shape + (-1,)).all(axis=-1)
            assert not bad.any(), report(scripts, bad, f"{cam}.{name}")


def test_rotations_within_the_float32_noise(device, restated):
    scripts = S.all_scripts()
    runs = restated["serial"]
    noise_q, noise_r = S.rotation_noise(runs)
    worst = {}
    for mode in MODES:
        got = device[mode]
        want = np.stack([r.states for r in restated[mode]])
        measured = np.array([S.is_measured(r) for r in restated[mode]])
        assert measured.sum() >= 100
        q64 = np.stack([r.q64 for r in restated[mode]])
        r64 = np.stack([r.R64 for r in restated[mode]])
        for what, g, w32, w64, noise in (("cam", got["cam"]["q_xyzw"], want["cam"]["q_xyzw"], q64[:, :, 0], noise_q),
                                         ("cam_new", got["cam_new"]["q_xyzw"], want["cam_new"]["q_xyzw"], q64[:, :, 1], noise_q),
                                         ("R", got["R"], want["R"], r64, noise_r)):
            # against the float32 restatement, every script: finite where it is finite, then within the bound
            finite = np.isfinite(w32)
            bad = (np.isfinite(g) != finite) | (np.isnan(g) != np.isnan(w32)) | (~finite & ~np.isnan(w32) & (g != w32))
            assert not bad.any(), report(scripts, bad.any(axis=-1), f"{mode} {what}: finiteness")
            err32 = np.where(finite, np.abs(np.where(finite, g, 0).astype(np.float64) - np.where(finite, w32, 0)), 0.0)
            # against the float64 shadow, the finite well-conditioned scripts
            err64 = np.abs(g[measured].astype(np.float64) - w64[measured])
            ratio32, ratio64 = float(err32.max() / (4 * noise)), float(err64.max() / (4 * noise))
            worst[f"{mode} {what}"] = (round(ratio32, 4), round(ratio64, 4))
            assert ratio32 <= 1, report(scripts, (err32 > 4 * noise).any(axis=-1), f"{mode} {what} vs float32 restatement, worst / bound {ratio32}")
            assert ratio64 <= 1, f"{mode} {what} vs float64 shadow: worst / bound {ratio64}"
    print(f"\nnoise: quaternion {noise_q:.4g}, R {noise_r:.4g}; worst |gpu - reference| / (4 x noise) as (float32 restatement on all "
          f"scripts, float64 shadow on the well-conditioned ones): {worst}")


def test_rounds_after_done_change_nothing(device):
    scripts = S.all_scripts()
    for mode, got in device.items():
        finished = 0
        for k in range(len(scripts)):
            if got["done"][k].any():
                first = int(np.argmax(got["done"][k]))
                later = got[k, first:]
                finished += len(later) > 1
                assert same_records(later, np.repeat(later[:1], len(later))).all(), (mode, scripts[k]["name"])
        assert finished >= 300, mode


def test_argument_checks():
    """every refusal returns PC_E_INVALID with a message and leaves the output alone (nothing was launched)"""
    L = hip.load()
    ctx = hip.Context(0)
    options, cameras, sums = pack(S.all_scripts()[:2])
    states = np.full((2, S.ROUNDS, hip.LM_DEBUG_STATE_WORDS), 0x5A5A5A5A, np.uint32)
    o, c, s, st = options.ctypes.data, cameras.ctypes.data, sums.ctypes.data, states.ctypes.data
    good = dict(ctx=ctx._h, mode=0, n_scripts=2, n_rounds=S.ROUNDS, max_rounds=100, options=o, initial=c, sums=s, states=st)
    refused = [dict(ctx=None), dict(options=None), dict(initial=None), dict(sums=None), dict(states=None), dict(mode=-1), dict(mode=3),
               dict(n_scripts=0), dict(n_scripts=-1), dict(n_scripts=1025), dict(n_rounds=0), dict(n_rounds=-1), dict(n_rounds=17)]
    for change in refused:
        a = dict(good, **change)
        rc = L.pc_debug_lm_decide(a["ctx"], a["mode"], a["n_scripts"], a["n_rounds"], a["max_rounds"], a["options"], a["initial"], a["sums"], a["states"])
        assert rc == -1, change                                   # PC_E_INVALID
        assert b"pc_debug_lm_decide" in L.pc_last_error(), change
        assert (states == 0x5A5A5A5A).all(), change
    assert L.pc_debug_lm_decide(*[good[k] for k in ("ctx", "mode", "n_scripts", "n_rounds", "max_rounds", "options", "initial", "sums", "states")]) == 0
    assert not (states == 0x5A5A5A5A).all()
    ctx.close()
