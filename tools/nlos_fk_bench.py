"""f-k migration at BASELINE config 4's capture shape: confocal, 256 x 256 scan points of a 2 x 2 wall, temporal_bins=4096,
bin_width_opl=2^-11, start_opl=1.85, bin_factor=4 (T' = 2000, a padded grid of 512 x 512 x 4000).  Device-event times after
warm-up, the median of the repeats, of
  * each of the three HIP passes (mtr_fk_prepare / mtr_fk_stolt / mtr_fk_finish) and each of the two FFTs (torch.fft),
  * the same three passes written in torch ops (meshgrid, gather, where) — alternating with the HIP pass they restate —,
  * the whole fk_migration call, and backproject(..., "linear") onto a slab of the same grid (its cost is linear in the
    depth rows: the slab's time and the figure scaled to the whole grid are both printed, named as such),
with each HIP pass's achieved bytes/s (the bytes the pass must move, from the shapes) against the HBM peak.
    python tools/nlos_fk_bench.py [H] [W] [T] [bin_factor] [repeats] [backproject_rows]
The capture is synthetic (point scatterers on a noise floor, seeded): the passes' times do not depend on its values."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12            # bytes/s, the MI355X's HBM3E specification; about 6.3e12 is what a float4 copy achieves


def timed(fn, reps, warm=2):
    """median, min and max of `reps` device-event times of fn(), in ms, after `warm` untimed calls"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def timed_pair(f, g, reps, warm=2):
    """two versions of one step, alternating inside the same window"""
    for _ in range(warm):
        f(), g()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(reps):
        for k, fn in enumerate((f, g)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b))
    return tuple((float(np.median(m)), float(min(m)), float(max(m))) for m in out)


def capture_for(H, W, T, bw, start, dev):
    g = torch.Generator(device="cpu").manual_seed(0)
    Y = 1e-3 * torch.rand((H, W, T), generator=g)
    xs = ((torch.arange(W) + 0.5) / W * 2 - 1)[None, :]
    ys = ((torch.arange(H) + 0.5) / H * 2 - 1)[:, None]
    for (px, py, pz, a) in ((0.3, -0.2, 1.0, 1.0), (-0.4, 0.5, 1.3, 0.5)):
        r = torch.sqrt((xs - px) ** 2 + (ys - py) ** 2 + pz ** 2)
        b = torch.floor((2 * r - start) / bw).long()
        ok = (b >= 0) & (b < T)
        yy, xx = torch.nonzero(ok, as_tuple=True)
        Y[yy, xx, b[yy, xx]] += (a / r ** 4)[yy, xx]
    return Y.to(dev)


def main():
    arg = [int(v) for v in sys.argv[1:]]
    H, W, T, q, reps, bp_rows = (arg + [256, 256, 4096, 4, 7, 4][len(arg):])[:6]
    assert torch.cuda.is_available(), "a timing needs the GPU"
    import mitransient_amd as mitr
    from mitransient_amd.nlos import CaptureGeometry, _fk_plan
    from mitransient_amd.runtime import get_context
    ctx = get_context()
    dev = torch.device("cuda", ctx.device_index)
    bw, start = 2.0 ** -11, 1.85
    pts = np.zeros((H, W, 3))
    pts[..., 0] = (((np.arange(W) + 0.5) / W) * 2 - 1)[None, :]
    pts[..., 1] = (((np.arange(H) + 0.5) / H) * 2 - 1)[:, None]
    geom = CaptureGeometry(2, pts, pts.reshape(-1, 3).copy(), np.zeros((H, W)), np.zeros(H * W), start, bw, T)
    plan = _fk_plan("nlos_fk_bench", geom, None, q)
    Tp, nz, z0 = plan.depth_bins, plan.nz, plan.z_begin
    d = plan.desc()
    ax, ay = float(d.ax), float(d.ay)
    print("capture %d x %d x %d, bin_factor %d: T' = %d, padded grid %d x %d x %d (%.2f GB as f32, %.2f GB as complex64), "
          "volume (%d, %d, %d)" % (H, W, T, q, Tp, 2 * H, 2 * W, 2 * Tp, 32e-9 * H * W * Tp, 64e-9 * H * W * Tp, nz, H, W))
    Y = capture_for(H, W, T, bw, start, dev)
    shift = torch.from_numpy(plan.shift).to(dev)

    def launch(entry, *tensors):
        ctx.bind_current_stream()
        ctx.check(getattr(ctx.lib, entry)(ctx.handle, C.byref(d), *(C.c_void_p(x.data_ptr()) for x in tensors)), entry)

    def rel(a, b):
        return float(torch.linalg.vector_norm((a - b).flatten()) / torch.linalg.vector_norm(b.flatten()))

    def report(name, hip, ops, nbytes, err):
        print("%-8s HIP %8.3f ms [%.3f .. %.3f]   torch ops %8.3f ms [%.3f .. %.3f]   ratio %.2fx   %.2f GB moved: %.2f TB/s, "
              "%.0f%% of the 8.0 TB/s HBM peak   (torch ops vs HIP rel-L2 %.1e)"
              % (name, hip[0], hip[1], hip[2], ops[0], ops[1], ops[2], ops[0] / hip[0], nbytes * 1e-9, nbytes / hip[0] * 1e-9,
                 100.0 * nbytes / (hip[0] * 1e-3) / HBM_PEAK, err))

    # ---- prepare
    padded = torch.empty((2 * H, 2 * W, 2 * Tp), dtype=torch.float32, device=dev)
    k = torch.arange(Tp, device=dev)
    ramp = (k.float() + 0.5) / float(Tp)

    def prepare_ops():
        S = torch.zeros((H, W, Tp), dtype=torch.float32, device=dev)
        for i in range(q):
            b = k[None, None, :] * q + i - shift[:, :, None].long()
            ok = (b >= 0) & (b < T)
            S = S + torch.where(ok, torch.gather(Y, 2, b.clamp(0, T - 1)), torch.zeros((), device=dev))
        P = torch.zeros((2 * H, 2 * W, 2 * Tp), dtype=torch.float32, device=dev)
        P[:H, :W, :Tp] = torch.sqrt(S.clamp_min(0.0)) * ramp
        return P
    hip, ops = timed_pair(lambda: launch("mtr_fk_prepare", Y, shift, padded), prepare_ops, reps)
    read = 4.0 * H * W * min(T, Tp * q) + 4.0 * H * W
    report("prepare", hip, ops, read + 4.0 * padded.numel(), rel(prepare_ops(), padded))

    # ---- the forward FFT
    t = timed(lambda: torch.fft.rfftn(padded), reps)
    tc = timed(lambda: torch.fft.rfftn(padded).contiguous(), reps)
    raw = torch.fft.rfftn(padded)
    print("rfftn    %8.3f ms [%.3f .. %.3f]   (torch.fft: %d x %d x %d real -> %d x %d x %d complex64, strides %s); made contiguous, as "
          "fk_migration takes it: %8.3f ms [%.3f .. %.3f]" % (t + (2 * H, 2 * W, 2 * Tp, 2 * H, 2 * W, Tp + 1, tuple(raw.stride())) + tc))
    spectrum = raw.contiguous()
    del raw
    del padded

    # ---- stolt
    resampled = torch.empty((2 * H, 2 * W, 2 * Tp), dtype=torch.complex64, device=dev)

    def signed(n2):
        i = torch.arange(n2, device=dev)
        return torch.where(i < n2 // 2, i, i - n2).float()

    def stolt_ops():
        ky, kx, kz = torch.meshgrid(signed(2 * H) / H, signed(2 * W) / W, signed(2 * Tp) / Tp, indexing="ij")
        kp = torch.sqrt((ax * kx) ** 2 + (ay * ky) ** 2 + kz ** 2)
        p = kp * Tp
        f = torch.floor(p)
        valid = (kz > 0) & (f + 1 <= Tp)
        i0 = f.long().clamp(0, Tp - 1)
        w = p - f
        G = ((1 - w) * torch.gather(spectrum, 2, i0) + w * torch.gather(spectrum, 2, i0 + 1)) * (kz / kp)
        return torch.where(valid, G, torch.zeros((), dtype=torch.complex64, device=dev))
    hip, ops = timed_pair(lambda: launch("mtr_fk_stolt", spectrum, resampled), stolt_ops, reps)
    report("stolt", hip, ops, 8.0 * spectrum.numel() + 8.0 * resampled.numel(), rel(torch.view_as_real(stolt_ops()), torch.view_as_real(resampled)))
    del spectrum

    # ---- the inverse FFT
    t = timed(lambda: torch.fft.ifftn(resampled), reps)
    tc = timed(lambda: torch.fft.ifftn(resampled).contiguous(), reps)
    raw = torch.fft.ifftn(resampled)
    print("ifftn    %8.3f ms [%.3f .. %.3f]   (torch.fft: %d x %d x %d complex64, strides %s); made contiguous: %8.3f ms [%.3f .. %.3f]"
          % (t + (2 * H, 2 * W, 2 * Tp, tuple(raw.stride())) + tc))
    field = raw.contiguous()
    del raw
    del resampled

    # ---- finish
    volume = torch.empty((nz, H, W), dtype=torch.float32, device=dev)

    def finish_ops():
        c = torch.view_as_real(field[:H, :W, z0:z0 + nz])
        return (c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]).permute(2, 0, 1).contiguous()
    hip, ops = timed_pair(lambda: launch("mtr_fk_finish", field, volume), finish_ops, reps)
    report("finish", hip, ops, 8.0 * H * W * nz + 4.0 * volume.numel(), rel(finish_ops(), volume))
    del field

    # ---- the whole call, and the direct sum it replaces
    t = timed(lambda: mitr.nlos.fk_migration(Y, geom, bin_factor=q), max(reps // 2, 3), warm=1)
    print("fk_migration, the whole call: %8.3f ms [%.3f .. %.3f]" % t)
    z = plan.depths()
    rows = min(bp_rows, nz)
    mid = nz // 2
    lo, hi = z[mid] - plan.dz / 2, z[mid + rows - 1] + plan.dz / 2
    t = timed(lambda: mitr.nlos.backproject(Y, geom, (-1.0, -1.0, lo), (1.0, 1.0, hi), (W, H, rows), "linear"), 3, warm=1)
    print("backproject(linear) onto %d of the grid's %d depth rows (%d x %d voxels each): %8.3f ms [%.3f .. %.3f]; scaled to all "
          "%d rows (the direct sum is linear in them; not measured whole): %.0f ms" % ((rows, nz, H, W) + t + (nz, t[0] * nz / rows)))


if __name__ == "__main__":
    main()
