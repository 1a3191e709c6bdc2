"""Every device ray walker against the host walk, ray by ray.  The library's ray-query harness (mitransient_amd/csrc/mtr_walk_kat.hip)
stages a scene the way a product kernel does and runs the instantiation of traverse() that kernel runs — wide_walk_device over the
8-wide tree in LDS (with the scene's leaf-pair trait and without), the quantised 8- and 4-wide trees in HBM, and flat_walk_device in
each of its forms: loading references, with top-level triangle leaves, over the child-ordered primitive table with one kernarg base,
and that with the SHADOW HULL tiers on — under BOTH of the Makefile's flag sets, on the ray families of tests/walk_cases.py: random
rays, cube edges and corners, shared diagonals, rectangle borders, tmax ties, second-nearest candidates, grazed spheres, shadow rays
built on the device, and one set of rays in many wave shapes.  Closest hit: t, u, v bits and the slot equal the host twin's
(tests/host_harness.cpp hh_walk) for every ray; any hit: the flag equals it.  tests/test_walk_cases.py holds that host walk to the
oracle and to f64 on the same rays and shows that the families reach their edges.  One child process per scene, under its own time
limit (tests/walk_gpu_cases.py); a child that did not end well stops the ones after it."""
import functools
import json
import os
import subprocess
import sys

import pytest

import walk_cases as W

HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = pytest.mark.gpu

_ENDED_BADLY = []          # a child that faulted, aborted or ran out of time: nothing more is started on that device by this module


@functools.lru_cache(maxsize=None)
def run_scene(name, timeout=180):
    if _ENDED_BADLY:
        pytest.fail(f"not started: the child of scene '{_ENDED_BADLY[0]}' did not end well")
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "walk_gpu_cases.py"), name], capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _ENDED_BADLY.append(name)
        raise
    if r.returncode != 0:
        _ENDED_BADLY.append(name)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("name", list(W.SCENES))
def test_every_form_ran_and_refusals_were_refused(name):
    """the run list equals the expected table — a form that silently did not run is a failure — and the hook launched nothing for a form
    the scene's traits do not allow, a scene that does not fit LDS, a flat form without a flat top level, a hull form without a hull,
    and n == 0: each with its own code"""
    out = run_scene(name)
    assert out["runs"] == W.expected_runs(name), [r for r in W.expected_runs(name) if r not in out["runs"]][:5]
    want = [[s, f, code] for s, f, code in W.REFUSALS if s == name] + [[name, "n=0", W.ERR_EMPTY]]
    assert out["refusals"] == want, out["refusals"]
    print(f"[walk] {name}: {len(out['runs'])} runs, {sum(r[4] for r in out['runs'])} rays, device seconds "
          + ", ".join(f"{k} {v:.3f}" for k, v in out["seconds"].items()))


CASES = [(s, f, x) for s in W.SCENES for f in W.SCENES[s][0] for x in W.SUFFIXES]


@pytest.mark.parametrize("name,form,suffix", CASES, ids=[f"{s}-{f}-{'kflags' if x else 'others'}" for s, f, x in CASES])
def test_device_walk_equals_host_walk_ray_by_ray(name, form, suffix):
    out = run_scene(name)
    ran = [r for r in out["runs"] if r[1] == form and r[2] == suffix]
    assert ran and sum(r[4] for r in ran) > 0, (name, form, suffix)
    bad = {k: v for k, v in out["failures"].items() if k.startswith(f"{form}|{suffix}|")}
    assert not bad, f"{name}, {form}, flag set '{suffix}': {len(bad)} families differ\n" + "\n".join(bad.values())


SHADOW = [(f, x) for f in W.SHADOW_FORMS for x in W.SUFFIXES]


@pytest.mark.xfail(strict=True, reason="a shadow ray whose origin lies IN a wall's plane (a surface standing on it: the offset stays in the plane) meets that "
                   "wall at t = -oz / dz with oz = +0.  IEEE 754 makes that -0 for dz > 0, and the MI355X returns 80000000; the host build and "
                   "the oracle return 00000000, because g++ folds the negation into the fused multiply-add that computes oz "
                   "(-(a b + c) as (-a) b - c: 1 - 1 = +0).  On the MI355X 552 of 24 576 shadow rays under either flag set, e.g. sp bee17793 "
                   "be973a0a bf800000 gn bf351b71 3f34ee73 00000000 (u1, u2) 3f16cf5a 3f05ffff: host t u v slot 00000000 bee18828 be972979 "
                   "00000014, device 80000000 bee18828 be972979 00000014.  Occlusion, u, v and the slot agree; t = +-0 is the same point "
                   "(HISTORY.md); the device is the one that follows the source")
@pytest.mark.parametrize("form,suffix", SHADOW, ids=[f"{f}-{'kflags' if x else 'others'}" for f, x in SHADOW])
def test_shadow_rays_closest_hit_words_equal_host(form, suffix):
    d = run_scene("cornell")["shadow_closest"][f"{form}|{suffix}"]
    assert d["differ"] == 0, d["first"]


@pytest.mark.parametrize("form,suffix", SHADOW, ids=[f"{f}-{'kflags' if x else 'others'}" for f, x in SHADOW])
def test_shadow_rays_closest_hit_differs_in_the_sign_of_a_zero_t_alone(form, suffix):
    """what does hold of the closest-hit words of the shadow family: wherever device and host differ, the host's t is +0, the device's
    -0, and u, v and the slot are equal — no other kind of difference"""
    d = run_scene("cornell")["shadow_closest"][f"{form}|{suffix}"]
    print(f"[walk] shadow closest hits, {form} '{suffix}': {d['differ']} of {d['of']} differ")
    assert d["only_the_sign_of_a_zero_t"], d["first"]
