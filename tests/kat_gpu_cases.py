"""One family of tests/test_gpu_kat.py, run in a child process of its own (the test gives it a time limit):
``python tests/kat_gpu_cases.py <family>`` runs every case of the family (tests/kat_cases.py) through the device harness of the
library — both flag sets, at the full size, n = 1 and n = 63 — and through the host twin, and prints one JSON line:
{"runs": ..., "words": ..., "failures": {"<case>|<suffix>": message}, "extra": {"safe_rcp|<suffix>": its distance from the host}}."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import kat_cases as K  # noqa: E402


def run_device(lib, suffix, case, n):
    """the outputs of mtr_test_dev_<entry><suffix> as uint32 arrays"""
    import torch
    ins = [torch.from_numpy(a.view(np.int32)).cuda() for a in case.inputs(n)]
    outs = [torch.zeros(s, dtype=torch.int32, device="cuda") for s in case.out_shapes(n)]
    fn = getattr(K.private_handle(lib), "mtr_test_dev_" + case.entry + suffix)
    fn.restype = C.c_int
    rc = case.invoke(fn, n, [t.data_ptr() for t in ins], [t.data_ptr() for t in outs])
    assert rc == 0, f"mtr_test_dev_{case.entry}{suffix}: hipError_t {rc}"
    torch.cuda.synchronize()
    return [t.cpu().numpy().view(np.uint32) for t in outs]


def family(name):
    import __graft_entry__ as g
    from mitransient_amd import _cabi
    lib = _cabi.load_library()
    hh = C.CDLL(g.build_host_harness())
    failures, extra, runs, words = {}, {}, 0, 0
    for case in K.cases(name):
        for n in (case.n,) + K.SMALL_N:
            host = case.run_cpu(hh, "hh_", n)
            for suffix in K.SUFFIXES:
                dev = run_device(lib, suffix, case, n)
                runs += 1
                words += sum(o.size for o in dev)
                msgs = [K.report(case, f"flag set '{suffix}'", host, dev, n)]
                if name == "pairs":          # <true> against <false> on the device itself
                    msgs.append(K.report(case, f"flag set '{suffix}', <true> against <false>", [dev[0][:8]], [dev[0][8:]], n, ("packed", "plain ")))
                msgs = [m for m in msgs if m]
                if msgs:
                    failures.setdefault(f"{case.name}|{suffix}", "\n".join(msgs))
                if case.name == "safe_rcp" and n == case.n:
                    extra[f"safe_rcp|{suffix}"] = K.safe_rcp_distance(host[0], dev[0])
    return {"runs": runs, "words": words, "failures": failures, "extra": extra}


if __name__ == "__main__":
    import torch
    torch.cuda.set_device(0)
    print(json.dumps(family(sys.argv[1])))
