"""One scene of tests/test_gpu_walk.py, run in a child process of its own (the test gives it a time limit):
``python tests/walk_gpu_cases.py <scene>`` puts the scene of tests/walk_cases.py on the device and asks every walker form the scene
has, under both flag sets, about every ray of the scene's families (mitransient_amd/csrc/mtr_walk_kat.hip), compares each answer with
the host twin's (tests/host_harness.cpp hh_walk, hh_walk_shadow) word for word, and prints one JSON line:
{"runs": [[scene, form, suffix, family, n]], "failures": {"form|suffix|family": message}, "refusals": [[scene, form, code]],
 "seconds": {"form|suffix": device time of its runs}, "shadow_closest": {"form|suffix": the closest-hit words of the shadow rays}}.  A launch that reports an error ends the child at once: nothing more is started on
that device."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import walk_cases as W  # noqa: E402


def hexs(a):
    return " ".join(f"{int(w):08x}" for w in np.atleast_1d(a).reshape(-1).view(np.uint32))


class Device:
    def __init__(self, name):
        import torch
        from mitransient_amd.runtime import get_context
        self.torch = torch
        self.ctx = get_context()
        self.lib = C.CDLL(self.ctx.lib._name)            # a handle of this module's own: its argtypes stay apart
        self.sd = W.scene(name)
        self.handle = C.c_void_p()
        desc = self.sd.desc()
        self.ctx.check(self.ctx.lib.mtr_scene_create(self.ctx.handle, C.byref(desc), C.byref(self.handle)), "mtr_scene_create")

    def hook(self, suffix):
        fn = getattr(self.lib, "mtr_test_dev_walk" + suffix)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64] + [C.c_void_p] * 5
        return fn

    def walk(self, form, suffix, o, d, tm):
        """(hit4, occ, seconds) of one launch; raises on any error code: the caller stops"""
        torch = self.torch
        n = len(o)
        ins = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in (o, d, tm)]
        hit4 = torch.full((n, 4), 0x55555555, dtype=torch.int32, device="cuda")
        occ = torch.full((n,), 0x55, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = self.hook(suffix)(self.handle, W.FORMS[form], n, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), hit4.data_ptr(), occ.data_ptr())
        if rc != 0:
            raise RuntimeError(f"mtr_test_dev_walk{suffix}(form {form}, n {n}) returned {rc}")
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return hit4.cpu().numpy().view(np.uint32), occ.cpu().numpy(), dt

    def refuse(self, form):
        """the hook's answer to a form it must not launch (n = 1 of valid memory is handed over all the same)"""
        torch = self.torch
        ins = [torch.zeros(4, dtype=torch.float32, device="cuda") for _ in range(3)]
        ins[1][2] = 1.0
        hit4 = torch.zeros(4, dtype=torch.int32, device="cuda")
        occ = torch.zeros(4, dtype=torch.uint8, device="cuda")
        return int(self.hook("")(self.handle, W.FORMS[form], 1, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), hit4.data_ptr(), occ.data_ptr()))


def compare(name, family, idx, host, dev, what):
    """None, or the message: the first three rays whose words differ, replayable"""
    (h4, hocc), (d4, docc) = host, dev
    bad = np.flatnonzero(np.any(h4 != d4, axis=1) | (hocc != docc))
    if not bad.size:
        return None
    lines = [f"{name} {what}: {bad.size} of {len(idx)} rays differ from the host walk"]
    for i in bad[:3]:
        lines.append(f"  {W.describe(name, family.split('/')[0], int(idx[i]))}\n    host   t u v slot {hexs(h4[i])} occ {int(hocc[i])}\n"
                     f"    device t u v slot {hexs(d4[i])} occ {int(docc[i])}")
    return "\n".join(lines)


def scene_runs(name):
    import __graft_entry__ as g
    hh = C.CDLL(g.build_host_harness())
    dev = Device(name)
    runs, failures, seconds = [], {}, {}
    host_cache = {}
    shadow_flags, shadow_closest = {}, {}
    refusals = [[s, f, dev.refuse(f)] for s, f, _ in W.REFUSALS if s == name]
    n_err = dev.hook("")(dev.handle, 0, 0, None, None, None, None, None)          # n == 0: refused in front of everything else
    refusals.append([name, "n=0", int(n_err)])
    for form in W.SCENES[name][0]:
        for suffix in W.SUFFIXES:
            for family in W.families_of(name, form):
                r = W.rays(name, family)
                base = None
                for var, idx in W.variants(r):
                    key = (family, var, W.TWIN[form])
                    if key not in host_cache:
                        host_cache[key] = W.host_answer(hh, name, family, form, var, idx)
                    if family == "shadow":
                        o, d, tm = r.o[idx], r.d[idx], r.tmax[idx]
                    else:
                        o, d, tm = W.variant_rays(r, var, idx)
                    d4, docc, dt = dev.walk(form, suffix, o, d, tm)
                    seconds[f"{form}|{suffix}"] = seconds.get(f"{form}|{suffix}", 0.0) + dt
                    runs.append([name, form, suffix, family + var, int(len(idx))])
                    if family == "shadow":
                        # any hit: the flag is what a shadow walk returns.  The closest-hit words of the same rays are reported apart
                        # ("shadow_closest": test_gpu_walk.py carries what differs there)
                        h4, hocc = host_cache[key]
                        msg = compare(name, family, idx, (h4 * 0, hocc), (d4 * 0, docc), f"{form} '{suffix}' shadow (occlusion)")
                        shadow_flags[(form, suffix)] = docc
                        bad = np.flatnonzero(np.any(h4 != d4, axis=1))
                        only_zero_sign = bool(np.all((h4[bad, 0] == 0) & (d4[bad, 0] == 0x80000000) & np.all(h4[bad, 1:] == d4[bad, 1:], axis=1)))
                        shadow_closest[f"{form}|{suffix}"] = {
                            "differ": int(bad.size), "of": int(len(idx)), "only_the_sign_of_a_zero_t": only_zero_sign,
                            "first": "" if not bad.size else f"{W.describe(name, 'shadow', int(bad[0]))}: host t u v slot {hexs(h4[bad[0]])}, device {hexs(d4[bad[0]])}"}
                    else:
                        msg = compare(name, family + var, idx, host_cache[key], (d4, docc), f"{form} '{suffix}' {family}{var}")
                    if family == "wave_shapes":
                        # per-ray words must not depend on n, on the order, or on what the other lanes of the wave do
                        if var == "":
                            base = (d4, docc)
                        else:
                            real = np.arange(len(idx))[W.LANE37::64] if var == "/lane37" else np.arange(len(idx))
                            same = np.all(base[0][idx[real]] == d4[real], axis=1) & (base[1][idx[real]] == docc[real])
                            if not same.all() and msg is None:
                                i = real[np.flatnonzero(~same)[0]]
                                msg = (f"{name} {form} '{suffix}' wave_shapes{var}: ray {int(idx[i])} answers {hexs(d4[i])} occ {int(docc[i])} here and "
                                       f"{hexs(base[0][idx[i]])} occ {int(base[1][idx[i]])} in the full run\n  {W.describe(name, 'wave_shapes', int(idx[i]))}")
                    if msg:
                        failures.setdefault(f"{form}|{suffix}|{family}", msg)
    for suffix in W.SUFFIXES:            # the HULL tiers return what the full stage returns
        a, b = shadow_flags.get(("flat_table_shadow", suffix)), shadow_flags.get(("flat_table_hull", suffix))
        if a is not None and b is not None and not np.array_equal(a, b):
            i = int(np.flatnonzero(a != b)[0])
            failures.setdefault(f"flat_table_hull|{suffix}|shadow-against-flat_table",
                                f"{name} '{suffix}': {int((a != b).sum())} shadow rays answer differently with the HULL tiers on; "
                                f"{W.describe(name, 'shadow', i)}: flat_table {int(a[i])}, flat_table_hull {int(b[i])}")
    return {"runs": runs, "failures": failures, "refusals": refusals, "seconds": seconds, "shadow_closest": shadow_closest}


if __name__ == "__main__":
    import torch
    torch.cuda.set_device(0)
    print(json.dumps(scene_runs(sys.argv[1])))
