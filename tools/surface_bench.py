"""hd95 / asd per case: the host route (scipy, utils/metrics.py) against the GPU route (csrc/surface.hip, utils/surface_gpu.py).

Shapes: two offset balls as one class at 112x112x80 (the LA patch) and 192x160x88 (an LA-sized whole case); an ACDC-like
10x256x256 label volume with classes 1..3.  Per shape:
  host        asd + hd95 of every class as the evaluation entry points call them with surface="host"   (time.perf_counter)
  gpu kernels surface_histograms between two device events (memset + the three passes, all classes in one call)
  gpu wall    surface_metrics on label volumes that are on the device (what test_single_volume has): kernels, torch.nonzero, the
              copy of the non-empty bins to the host and the float64 finish
  gpu wall+up the same from numpy arrays (what test_all_case has): the upload of both volumes included
Medians of --reps runs after --warmup runs.  The two routes' results are compared before anything is timed (hd95 ==, asd to 1e-12).

With --spacing SZ SY SX and / or --connectivity K (1..3) the same shapes are measured on the float64 record route instead
(csrc/surface.hip, surface_gpu.spaced_*): the host is metrics.binary with the same two arguments, "gpu kernels" is spaced_launch
between two device events, "gpu wall" is spaced_metrics on device labels (kernels, the copy of the records, sort and finish), and one
more column gives the unit-spacing integer route (surface_metrics from numpy arrays) on the same box for scale.  The routes are compared
first (hd95 and asd within 1e-12).

  python tools/surface_bench.py [--reps 10 --warmup 3 --host-reps 5] [--spacing 10 1.25 1.25] [--connectivity 1] [--out surface_bench_table.md]
--out writes the table and the line under it, nothing else.  profiles/surface_gpu_notes.md quotes such a table inside notes written
by hand; the tool refuses to overwrite that file."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from arco_amd.utils import metrics, surface_gpu


def ball(shape, centre, radius):
    g = np.indices(shape).astype(np.float64)
    return sum((g[i] - centre[i]) ** 2 for i in range(len(shape))) < radius * radius


def two_balls(shape):
    c = [s / 2 for s in shape]
    r = min(shape)
    return ball(shape, c, 0.35 * r).astype(np.int64), ball(shape, [x + 2 for x in c], 0.33 * r).astype(np.int64), [1]


def acdc_like(shape=(10, 256, 256)):
    """Three nested structures per slice (ring, ring, disc), the prediction shifted and a little smaller."""
    def vol(shift, scale):
        lab = np.zeros(shape, dtype=np.int64)
        for z in range(shape[0]):
            c = (shape[1] / 2 + shift + 0.5 * z, shape[2] / 2 - shift)
            for cls, r in ((1, 60), (2, 42), (3, 28)):
                lab[z][ball(shape[1:], c, r * scale)] = cls
        return lab
    return vol(3, 0.96), vol(0, 1.0), [1, 2, 3]


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def kernel_ms(p, g, classes, reps, warmup):
    ts = []
    for i in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        surface_gpu.surface_histograms(p, g, classes)
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def spaced_kernel_ms(p, g, classes, spacing, connectivity, reps, warmup):
    ts = []
    for i in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        surface_gpu.spaced_launch(p, g, classes, spacing, connectivity)
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def spaced_main(args, shapes, dev):
    """The table of the record route for --spacing / --connectivity."""
    spacing, conn = args.spacing, args.connectivity
    rows = []
    for name, (pred, gt, classes) in shapes:
        def host():
            return [(metrics.binary.hd95(pred == c, gt == c, spacing, conn), metrics.binary.asd(pred == c, gt == c, spacing, conn))
                    for c in classes]
        p, g = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
        exp, got = host(), surface_gpu.spaced_metrics(p, g, classes, spacing, conn)
        for (hd_h, asd_h), (hd_g, asd_g) in zip(exp, got):
            assert abs(hd_g - hd_h) <= 1e-12 * abs(hd_h) and abs(asd_g - asd_h) <= 1e-12 * abs(asd_h), (name, exp, got)
        n_rec = int(surface_gpu.spaced_launch(p, g, classes, spacing, conn)[2].item())
        t_host = median_ms(host, args.host_reps, 1)
        t_kern = spaced_kernel_ms(p, g, classes, spacing, conn, args.reps, args.warmup)
        t_wall = median_ms(lambda: surface_gpu.spaced_metrics(p, g, classes, spacing, conn), args.reps, args.warmup)
        t_up = median_ms(lambda: surface_gpu.spaced_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), classes, spacing,
                                                            conn), args.reps, args.warmup)
        t_int = median_ms(lambda: surface_gpu.surface_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), classes),
                          args.reps, args.warmup)
        rows.append((name, n_rec, t_host, t_kern, t_wall, t_up, t_int, exp))
        print("%-26s %7d records | host %9.1f ms | gpu kernels %7.3f ms, wall %7.2f ms, wall + upload %7.2f ms | x%.0f | integer route "
              "(unit spacing, connectivity 1) wall + upload %7.2f ms" % (name, n_rec, t_host, t_kern, t_wall, t_up, t_host / t_up, t_int),
              flush=True)
    lines = ["| Volume | records | host (scipy) | GPU kernels | GPU wall (labels on the device) | GPU wall + upload | host / GPU wall + upload | "
             "integer route wall + upload |", "|---|---|---|---|---|---|---|---|"]
    for name, n_rec, t_host, t_kern, t_wall, t_up, t_int, _ in rows:
        lines.append("| %s | %d | %.1f ms | %.3f ms | %.2f ms | %.2f ms | %.0fx | %.2f ms |" %
                     (name, n_rec, t_host, t_kern, t_wall, t_up, t_host / t_up, t_int))
    table = "\n".join(lines)
    note = ("voxelspacing %s, connectivity %d.  Host CPU: %s; GPU: %s.  Medians: host %d runs after 1, GPU %d runs after %d.  hd95 and asd "
            "within 1e-12 between the routes at every shape: %s." %
            (spacing, conn, cpu_model(), torch.cuda.get_device_name(0), args.host_reps, args.reps, args.warmup,
             "; ".join("%s hd95 %s asd %s" % (r[0].split(",")[0], ["%.4f" % m[0] for m in r[7]], ["%.4f" % m[1] for m in r[7]]) for r in rows)))
    return table, note


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown CPU"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--spacing", type=float, nargs=3, default=None, metavar=("SZ", "SY", "SX"),
                    help="voxel spacing: measure the float64 record route (surface_gpu.spaced_metrics) against metrics.binary with it")
    ap.add_argument("--connectivity", type=int, default=1, choices=(1, 2, 3), help="border connectivity; other than 1 selects the record route")
    ap.add_argument("--out", default=None, help="also write the table to this file (not profiles/surface_gpu_notes.md)")
    args = ap.parse_args()
    if args.out and os.path.basename(args.out) == "surface_gpu_notes.md":
        raise SystemExit("surface_bench: profiles/surface_gpu_notes.md is written by hand around a table of this tool; give --out another file")
    if not torch.cuda.is_available():
        raise SystemExit("surface_bench: needs the GPU (there is nothing to compare without it)")
    dev = "cuda:0"
    shapes = (("112x112x80, 1 class", two_balls((112, 112, 80))),
              ("192x160x88, 1 class", two_balls((192, 160, 88))),
              ("10x256x256, classes 1..3", acdc_like()))
    if args.spacing is not None or args.connectivity != 1:
        args.spacing = tuple(args.spacing) if args.spacing is not None else None
        table, note = spaced_main(args, shapes, dev)
        print(table + "\n\n" + note)
        if args.out:
            with open(args.out, "w") as f:
                f.write(table + "\n\n" + note + "\n")
        return
    rows = []
    for name, (pred, gt, classes) in shapes:
        def host():
            return [(metrics.binary.hd95(pred == c, gt == c), metrics.binary.asd(pred == c, gt == c)) for c in classes]
        p, g = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
        exp, got = host(), surface_gpu.surface_metrics(p, g, classes)
        for (hd_h, asd_h), (hd_g, asd_g) in zip(exp, got):
            assert hd_g == hd_h and abs(asd_g - asd_h) <= 1e-12 * abs(asd_h), (name, exp, got)
        t_host = median_ms(host, args.host_reps, 1)
        t_kern = kernel_ms(p, g, classes, args.reps, args.warmup)
        t_wall = median_ms(lambda: surface_gpu.surface_metrics(p, g, classes), args.reps, args.warmup)
        t_up = median_ms(lambda: surface_gpu.surface_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), classes),
                         args.reps, args.warmup)
        rows.append((name, t_host, t_kern, t_wall, t_up, exp))
        print("%-26s host %9.1f ms | gpu kernels %7.3f ms, wall %7.2f ms, wall + upload %7.2f ms | x%.0f" %
              (name, t_host, t_kern, t_wall, t_up, t_host / t_up), flush=True)
    lines = ["| Volume | host (scipy) | GPU kernels | GPU wall (labels on the device) | GPU wall + upload | host / GPU wall + upload |",
             "|---|---|---|---|---|---|"]
    for name, t_host, t_kern, t_wall, t_up, _ in rows:
        lines.append("| %s | %.1f ms | %.3f ms | %.2f ms | %.2f ms | %.0fx |" % (name, t_host, t_kern, t_wall, t_up, t_host / t_up))
    table = "\n".join(lines)
    note = ("Host CPU: %s; GPU: %s.  Medians: host %d runs after 1, GPU %d runs after %d.  hd95 equal (==) and asd within 1e-12 "
            "between the routes at every shape: %s." %
            (cpu_model(), torch.cuda.get_device_name(0), args.host_reps, args.reps, args.warmup,
             "; ".join("%s hd95 %s asd %s" % (r[0].split(",")[0], ["%.4f" % m[0] for m in r[5]], ["%.4f" % m[1] for m in r[5]]) for r in rows)))
    print(table + "\n\n" + note)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n\n" + note + "\n")


if __name__ == "__main__":
    main()
