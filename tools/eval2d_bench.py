"""One 2-D evaluation case with the zoom round trip on the host against the same case with it on the GPU, and the two zoom kernels
alone (csrc/zoom.hip, utils/zoom_gpu.py).

Per volume (10x256x216, 12x320x300, 10x512x512; patch 256x256, 4 classes; the package's U-Net in eval mode with random weights, an
image of noisy discs and labels of the same discs):
  case     wall time of eval_surface.test_single_volume(surface="gpu", zoom=...) for zoom="host" (test_2D.predict_volume: scipy's
           zoom(order=0) twice per slice, the arg-max map to the host and the prediction back up) and zoom="gpu", the two alternating
           in the same process, each call ended by a device synchronise                                      (time.perf_counter)
  kernels  zoom_gpu.zoom_nearest of the float32 volume to the patch and zoom_gpu.argmax_zoom_back of the logits to the slices' size,
           each between two device events; next to them scipy's zoom over the same slices on the host
Medians after warm-up.  Before anything is timed the two routes are compared: the same label map (array_equal) and the same metrics (==).
--order 3 adds, per volume, the same case with the cubic-spline zoom of the slices (order=3, the reference's test.py:116-135) on the
host route and on the gpu route, next to the order-0 gpu route of the same process, and the three kernels of zoom_gpu.zoom_cubic alone
(the two prefilter passes and the interpolation) next to the bytes each must move and scipy's zoom(order=3) of the same slices.
--act-dtype f16 adds, per volume, the zoom="gpu" case at act_dtype="f32" and at act_dtype="f16" (the forwards inside ops.eval_half,
the stored f16 logits read by arco_argmax_zoom_back2d_h), the two alternating in one process, with the calls of library entry points
one case makes on either route and the network forward of the case's slices alone on either route.

Every step runs in a child process of its own under --step-timeout seconds; the first step that fails or runs out of time ends the
run (nothing more is started on the GPU after it).

  python tools/eval2d_bench.py [--order 3] [--act-dtype f16] [--reps 10 --warmup 3 --kernel-reps 50 --step-timeout 300] [--out eval2d_bench_table.md]
--out writes the tables and the line under them, nothing else.  profiles/eval2d_gpu_notes.md quotes such tables inside notes written
by hand; the tool refuses to overwrite that file."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SHAPES = {"10x256x216": (10, 256, 216), "12x320x300": (12, 320, 300), "10x512x512": (10, 512, 512)}
PATCH, CLASSES = (256, 256), 4
TAG = "EVAL2D_BENCH "


def make_case(shape):
    """(image float32, label int64): per slice three discs of classes 1..3, the image their class plus noise."""
    rng = np.random.default_rng(sum(shape))
    S, x, y = shape
    g0, g1 = np.indices((x, y)).astype(np.float64)
    lab = np.zeros(shape, dtype=np.int64)
    for s in range(S):
        for c in range(1, CLASSES):
            c0, c1, r = rng.uniform(0.2, 0.8) * x, rng.uniform(0.2, 0.8) * y, rng.uniform(0.08, 0.2) * min(x, y)
            lab[s][(g0 - c0) ** 2 + (g1 - c1) ** 2 < r * r] = c
    img = (lab / (CLASSES - 1) + 0.3 * rng.standard_normal(shape)).astype(np.float32)
    return img, lab


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown CPU"


def event_ms(fn, reps, warmup):
    import torch
    ts = []
    for i in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def _net():
    import torch
    from arco_amd.networks.unetWithArgs import UNet
    torch.manual_seed(0)
    return UNet(1, CLASSES).cuda().eval()


# ---- the steps (each in a child process) ------------------------------------------------------------------------------------------------
def step_case(shape_name, args):
    import torch
    from arco_amd import eval_surface, test_2D
    img, lab = make_case(SHAPES[shape_name])
    net = _net()
    host_pred = test_2D.predict_volume(img, net, PATCH)
    assert np.array_equal(eval_surface.predict_volume(img, net, PATCH, zoom="gpu").cpu().numpy(), host_pred)
    metrics = {z: eval_surface.test_single_volume(img, lab, net, CLASSES, PATCH, surface="gpu", zoom=z) for z in ("host", "gpu")}
    assert metrics["host"] == metrics["gpu"], metrics
    ts = {"host": [], "gpu": []}
    for i in range(args.warmup + args.reps):
        for z in ("host", "gpu"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eval_surface.test_single_volume(img, lab, net, CLASSES, PATCH, surface="gpu", zoom=z)
            torch.cuda.synchronize()
            if i >= args.warmup:
                ts[z].append(time.perf_counter() - t0)
    return dict(shape=shape_name, host=statistics.median(ts["host"]) * 1e3, gpu=statistics.median(ts["gpu"]) * 1e3,
                host_min=min(ts["host"]) * 1e3, gpu_min=min(ts["gpu"]) * 1e3, classes_predicted=int(len(np.unique(host_pred))),
                dice=[float(m[0]) for m in metrics["gpu"]], dev=torch.cuda.get_device_name(0))


def step_kernels(shape_name, args):
    import torch
    from scipy.ndimage import zoom
    from arco_amd.utils import zoom_gpu
    S, x, y = SHAPES[shape_name]
    img, _ = make_case(SHAPES[shape_name])
    vol = torch.from_numpy(img).cuda()
    torch.manual_seed(1)
    logits = torch.randn((S, PATCH[0], PATCH[1], CLASSES), device="cuda").permute(0, 3, 1, 2)        # channels-last, as the net leaves them
    amax = logits.argmax(dim=1).cpu().numpy()
    t_fwd = event_ms(lambda: zoom_gpu.zoom_nearest(vol, PATCH), args.kernel_reps, args.warmup)
    t_back = event_ms(lambda: zoom_gpu.argmax_zoom_back(logits, (x, y)), args.kernel_reps, args.warmup)
    h_fwd, h_back = [], []
    for i in range(1 + args.reps):
        t0 = time.perf_counter()
        for s in range(S):
            zoom(img[s], (PATCH[0] / x, PATCH[1] / y), order=0)
        t1 = time.perf_counter()
        for s in range(S):
            zoom(amax[s], (x / PATCH[0], y / PATCH[1]), order=0)
        t2 = time.perf_counter()
        if i:
            h_fwd.append(t1 - t0)
            h_back.append(t2 - t1)
    return dict(shape=shape_name, fwd=t_fwd, back=t_back, host_fwd=statistics.median(h_fwd) * 1e3, host_back=statistics.median(h_back) * 1e3,
                fwd_bytes=4 * S * (x * y + PATCH[0] * PATCH[1]), back_bytes=S * (8 * x * y + 4 * CLASSES * min(x, PATCH[0]) * min(y, PATCH[1])))


def step_case3(shape_name, args):
    """One case with order=3 on the host route and on the gpu route, and with order=0 on the gpu route, alternating."""
    import torch
    from arco_amd import eval_surface
    img, lab = make_case(SHAPES[shape_name])
    net = _net()
    routes = {"host3": dict(zoom="host", order=3), "gpu3": dict(zoom="gpu", order=3), "gpu0": dict(zoom="gpu", order=0)}
    host_pred = eval_surface.predict_volume(img, net, PATCH, **routes["host3"])
    same_map = bool(np.array_equal(eval_surface.predict_volume(img, net, PATCH, **routes["gpu3"]).cpu().numpy(), host_pred))
    metrics = {k: eval_surface.test_single_volume(img, lab, net, CLASSES, PATCH, surface="gpu", **kw) for k, kw in routes.items()}
    ts = {k: [] for k in routes}
    for i in range(args.warmup + args.reps):
        for k, kw in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eval_surface.test_single_volume(img, lab, net, CLASSES, PATCH, surface="gpu", **kw)
            torch.cuda.synchronize()
            if i >= args.warmup:
                ts[k].append(time.perf_counter() - t0)
    inp = torch.randn((img.shape[0], 1) + PATCH, device="cuda")
    with torch.no_grad():
        t_net = event_ms(lambda: net(inp), args.reps, args.warmup)         # the network forward of the case's slices, for scale
    res = dict(shape=shape_name, same_map=same_map, same_metrics=metrics["host3"] == metrics["gpu3"], net=t_net,
               differs_from_order0=bool(metrics["gpu3"] != metrics["gpu0"]), dev=torch.cuda.get_device_name(0))
    for k in routes:
        res[k], res[k + "_min"] = statistics.median(ts[k]) * 1e3, min(ts[k]) * 1e3
    return res


def step_kernels3(shape_name, args):
    """The three launches of zoom_gpu.zoom_cubic, each alone between device events on preallocated buffers, and scipy's zoom(order=3)."""
    import torch
    from scipy.ndimage import zoom
    import arco_amd._lib as L
    from arco_amd.utils import zoom_gpu
    S, x, y = SHAPES[shape_name]
    img, _ = make_case(SHAPES[shape_name])
    vol = torch.from_numpy(img).cuda()
    coef = torch.empty((S, x, y), dtype=torch.float64, device="cuda")
    out = torch.empty((S,) + PATCH, dtype=torch.float32, device="cuda")
    consts = zoom_gpu.spline_constants(x, y)
    z0, z1 = (x - 1) / (PATCH[0] - 1), (y - 1) / (PATCH[1] - 1)
    t_cols = event_ms(lambda: L.call("arco_spline_prefilter2d", L.ptr(vol), S, x, y, *consts, 1, L.ptr(coef)), args.kernel_reps, args.warmup)
    t_rows = event_ms(lambda: L.call("arco_spline_prefilter2d", L.ptr(vol), S, x, y, *consts, 2, L.ptr(coef)), args.kernel_reps, args.warmup)
    t_int = event_ms(lambda: L.call("arco_zoom_cubic2d", L.ptr(coef), S, x, y, PATCH[0], PATCH[1], z0, z1, L.ptr(out)), args.kernel_reps,
                     args.warmup)
    t_all = event_ms(lambda: zoom_gpu.zoom_cubic(vol, PATCH), args.kernel_reps, args.warmup)
    host = []
    for i in range(1 + args.reps):
        t0 = time.perf_counter()
        for s in range(S):
            zoom(img[s], (PATCH[0] / x, PATCH[1] / y), order=3)
        if i:
            host.append(time.perf_counter() - t0)
    n = S * x * y
    return dict(shape=shape_name, cols=t_cols, rows=t_rows, interp=t_int, all=t_all, host=statistics.median(host) * 1e3,
                cols_bytes=(4 + 8) * n, rows_bytes=(8 + 8) * n, interp_bytes=8 * n + 4 * S * PATCH[0] * PATCH[1], lines_cols=S * y, lines_rows=S * x)


def step_caseh(shape_name, args):
    """One zoom="gpu" case at act_dtype="f32" and at "f16", alternating; the library entry points one case calls; the forward alone."""
    import torch
    import arco_amd._lib as L
    from arco_amd import eval_surface, ops
    img, lab = make_case(SHAPES[shape_name])
    net = _net()
    routes = {"f32": dict(zoom="gpu", act_dtype="f32"), "f16": dict(zoom="gpu", act_dtype="f16")}
    maps = {k: eval_surface.predict_volume(img, net, PATCH, **kw) for k, kw in routes.items()}
    metrics = {k: eval_surface.test_single_volume(img, lab, net, CLASSES, PATCH, surface="gpu", **kw) for k, kw in routes.items()}
    calls, real_call = {}, L.call
    for k, kw in routes.items():                       # counted outside the timed runs
        n = [0]

        def counting(name, *a, _n=n):
            _n[0] += 1
            return real_call(name, *a)
        L.call = counting
        try:
            eval_surface.test_single_volume(img, lab, net, CLASSES, PATCH, surface="gpu", **kw)
        finally:
            L.call = real_call
        calls[k] = n[0]
    ts = {k: [] for k in routes}
    for i in range(args.warmup + args.reps):
        for k, kw in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eval_surface.test_single_volume(img, lab, net, CLASSES, PATCH, surface="gpu", **kw)
            torch.cuda.synchronize()
            if i >= args.warmup:
                ts[k].append(time.perf_counter() - t0)
    inp = torch.randn((img.shape[0], 1) + PATCH, device="cuda")
    with torch.no_grad():
        t_net32 = event_ms(lambda: net(inp), args.kernel_reps, args.warmup)
        with ops.eval_half(logits="stored"):
            t_net16 = event_ms(lambda: net(inp), args.kernel_reps, args.warmup)
    res = dict(shape=shape_name, net32=t_net32, net16=t_net16, calls32=calls["f32"], calls16=calls["f16"],
               labels_differ=float((maps["f32"] != maps["f16"]).float().mean()), dice32=[float(m[0]) for m in metrics["f32"]],
               dice16=[float(m[0]) for m in metrics["f16"]], dev=torch.cuda.get_device_name(0))
    for k in routes:
        res[k], res[k + "_min"] = statistics.median(ts[k]) * 1e3, min(ts[k]) * 1e3
    return res


STEPS = {"case": step_case, "kernels": step_kernels, "case3": step_case3, "kernels3": step_kernels3, "caseh": step_caseh}


def steps(order=0, act_dtype="f32"):
    for kind in ("case", "kernels") + (("case3", "kernels3") if order == 3 else ()) + (("caseh",) if act_dtype == "f16" else ()):
        for s in SHAPES:
            yield "%s|%s" % (kind, s)


def run_step(name, args):
    kind, shape = name.split("|")
    print(TAG + json.dumps(STEPS[kind](shape, args)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--step-timeout", type=float, default=300.0, help="seconds for each step (a child process of its own)")
    ap.add_argument("--order", type=int, default=0, choices=(0, 3), help="3: also the order-3 (cubic-spline) case and kernel rows")
    ap.add_argument("--act-dtype", default="f32", choices=("f32", "f16"), help="f16: also the zoom=\"gpu\" case at act_dtype f32 and f16")
    ap.add_argument("--out", default=None, help="also write the tables to this file (not profiles/eval2d_gpu_notes.md)")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return run_step(args.step, args)
    if args.out and os.path.basename(args.out) == "eval2d_gpu_notes.md":
        raise SystemExit("eval2d_bench: profiles/eval2d_gpu_notes.md is written by hand around the tables of this tool; give --out another file")
    case_rows, kernel_rows, case3_rows, kernel3_rows, caseh_rows = [], [], [], [], []
    for name in steps(args.order, args.act_dtype):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps), "--warmup", str(args.warmup),
               "--kernel-reps", str(args.kernel_reps)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired as e:
            print(e.stdout or "")
            raise SystemExit("eval2d_bench: step %r ran past %.0f s; nothing more is started" % (name, args.step_timeout))
        found = [json.loads(l[len(TAG):]) for l in p.stdout.splitlines() if l.startswith(TAG)]
        if p.returncode != 0 or len(found) != 1:
            print(p.stdout)
            raise SystemExit("eval2d_bench: step %r failed with exit status %d; nothing more is started" % (name, p.returncode))
        r = found[0]
        if name.startswith("caseh"):
            caseh_rows.append(r)
            print("%-11s zoom=gpu per case: act_dtype f32 %8.2f ms, f16 %8.2f ms; net forward f32 %.3f ms, f16 %.3f ms; entry calls %d / %d" %
                  (r["shape"], r["f32"], r["f16"], r["net32"], r["net16"], r["calls32"], r["calls16"]), flush=True)
        elif name.startswith("case3"):
            case3_rows.append(r)
            print("%-11s order 3 per case: zoom=host %8.2f ms, zoom=gpu %8.2f ms; order 0 zoom=gpu %8.2f ms; net forward %.2f ms" %
                  (r["shape"], r["host3"], r["gpu3"], r["gpu0"], r["net"]), flush=True)
        elif name.startswith("kernels3"):
            kernel3_rows.append(r)
            print("%-11s prefilter axis 0 %.4f ms, axis 1 %.4f ms, interpolation %.4f ms, zoom_cubic %.4f ms, scipy %.1f ms" %
                  (r["shape"], r["cols"], r["rows"], r["interp"], r["all"], r["host"]), flush=True)
        elif name.startswith("case"):
            case_rows.append(r)
            print("%-11s test_single_volume per case: zoom=host %8.2f ms, zoom=gpu %8.2f ms" % (r["shape"], r["host"], r["gpu"]), flush=True)
        else:
            kernel_rows.append(r)
            print("%-11s to the patch: gpu %.4f ms, scipy %.1f ms | back: gpu %.4f ms, scipy %.1f ms" %
                  (r["shape"], r["fwd"], r["host_fwd"], r["back"], r["host_back"]), flush=True)
    lines = ["| Volume | test_single_volume per case, zoom=\"host\" | zoom=\"gpu\" | difference | host / gpu |", "|---|---|---|---|---|"]
    for r in case_rows:
        lines.append("| %s | %.2f ms | %.2f ms | %.2f ms | %.2fx |" % (r["shape"], r["host"], r["gpu"], r["host"] - r["gpu"], r["host"] / r["gpu"]))
    lines += ["", "| Volume | zoom_nearest to the patch | scipy, same slices | argmax_zoom_back | scipy zoom of the arg-max map |", "|---|---|---|---|---|"]
    for r in kernel_rows:
        lines.append("| %s | %.4f ms (%.0f GB/s) | %.1f ms | %.4f ms (%.0f GB/s) | %.1f ms |" %
                     (r["shape"], r["fwd"], r["fwd_bytes"] / r["fwd"] / 1e6, r["host_fwd"], r["back"], r["back_bytes"] / r["back"] / 1e6,
                      r["host_back"]))
    table = "\n".join(lines)
    note = ("Host CPU: %s; GPU: %s.  Medians: a case %d runs after %d, the two routes alternating (fastest runs: %s); a kernel %d launches "
            "after %d, between device events, the allocation of its output included; scipy %d runs after 1.  Patch %dx%d, %d classes, U-Net "
            "with random weights in eval mode (classes predicted: %s).  GB/s: bytes the kernel must move (source and output; for the way "
            "back the distinct logits rows that are sampled and the int64 labels) over its time.  zoom=\"gpu\" gave the label map of zoom=\"host\" "
            "(array_equal) and the same metrics (==) at every volume." %
            (cpu_model(), case_rows[0]["dev"], args.reps, args.warmup,
             "; ".join("%s %.2f / %.2f ms" % (r["shape"], r["host_min"], r["gpu_min"]) for r in case_rows), args.kernel_reps, args.warmup,
             args.reps, PATCH[0], PATCH[1], CLASSES, ", ".join("%s %d" % (r["shape"], r["classes_predicted"]) for r in case_rows)))
    if args.order == 3:
        lines = ["", "| Volume | order=3, zoom=\"host\" | order=3, zoom=\"gpu\" | order=0, zoom=\"gpu\" | host3 / gpu3 | net forward of the case |",
                 "|---|---|---|---|---|---|"]
        for r in case3_rows:
            lines.append("| %s | %.2f ms | %.2f ms | %.2f ms | %.2fx | %.2f ms |" % (r["shape"], r["host3"], r["gpu3"], r["gpu0"],
                                                                                r["host3"] / r["gpu3"], r["net"]))
        lines += ["", "| Volume | prefilter axis 0 (lines) | prefilter axis 1 (lines) | interpolation | zoom_cubic, all three | scipy zoom(order=3), same slices |",
                  "|---|---|---|---|---|---|"]
        for r in kernel3_rows:
            lines.append("| %s | %.4f ms, floor %.2f MB (%.0f GB/s), %d | %.4f ms, floor %.2f MB (%.0f GB/s), %d | %.4f ms, floor %.2f MB (%.0f GB/s) | "
                         "%.4f ms | %.1f ms |" %
                         (r["shape"], r["cols"], r["cols_bytes"] / 1e6, r["cols_bytes"] / r["cols"] / 1e6, r["lines_cols"], r["rows"],
                          r["rows_bytes"] / 1e6, r["rows_bytes"] / r["rows"] / 1e6, r["lines_rows"], r["interp"], r["interp_bytes"] / 1e6,
                          r["interp_bytes"] / r["interp"] / 1e6, r["all"], r["host"]))
        table += "\n" + "\n".join(lines)
        note += ("\n\nOrder 3: the three routes alternate in one process (fastest runs: %s).  zoom=\"gpu\", order=3 gave the label map of "
                 "zoom=\"host\", order=3: %s; the same metrics: %s; metrics other than order 0's: %s.  Byte floor of a kernel: every array it reads "
                 "or writes counted once (float32 in and float64 out for axis 0; float64 in and out for axis 1; float64 in and float32 out "
                 "for the interpolation); the kernels are timed on preallocated buffers, zoom_cubic with its two allocations." %
                 ("; ".join("%s %.2f / %.2f / %.2f ms" % (r["shape"], r["host3_min"], r["gpu3_min"], r["gpu0_min"]) for r in case3_rows),
                  ", ".join("%s %s" % (r["shape"], "yes" if r["same_map"] else "NO") for r in case3_rows),
                  ", ".join("%s %s" % (r["shape"], "yes" if r["same_metrics"] else "NO") for r in case3_rows),
                  ", ".join("%s %s" % (r["shape"], "yes" if r["differs_from_order0"] else "no") for r in case3_rows)))
    if args.act_dtype == "f16":
        lines = ["", "| Volume | zoom=\"gpu\", act_dtype=\"f32\" | zoom=\"gpu\", act_dtype=\"f16\" | f32 / f16 | entry-point calls per case, f32 | f16 | "
                 "net forward of the case, f32 | f16 |", "|---|---|---|---|---|---|---|---|"]
        for r in caseh_rows:
            lines.append("| %s | %.2f ms | %.2f ms | %.2fx | %d | %d | %.3f ms | %.3f ms |" %
                         (r["shape"], r["f32"], r["f16"], r["f32"] / r["f16"], r["calls32"], r["calls16"], r["net32"], r["net16"]))
        table += "\n" + "\n".join(lines)
        note += ("\n\nact_dtype: the two routes alternate in one process (fastest runs, f32 / f16: %s).  Entry-point calls: the calls of "
                 "library entry points (_lib.call) one test_single_volume makes, counted in a run of its own - an entry point may launch "
                 "more than one kernel, and torch's own launches (the rsqrt of the running variances, copies, the cat of the fp32 eval "
                 "route) are not in it.  Net forward: the eval-mode forward of the case's slices alone, median of %d between device "
                 "events.  Share of the label map that differs between the two routes: %s; dice per class f32 / f16: %s." %
                 ("; ".join("%s %.2f / %.2f ms" % (r["shape"], r["f32_min"], r["f16_min"]) for r in caseh_rows), args.kernel_reps,
                  ", ".join("%s %.2e" % (r["shape"], r["labels_differ"]) for r in caseh_rows),
                  "; ".join("%s %s / %s" % (r["shape"], ["%.4f" % d for d in r["dice32"]], ["%.4f" % d for d in r["dice16"]]) for r in caseh_rows)))
    print(table + "\n\n" + note)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n\n" + note + "\n")


if __name__ == "__main__":
    main()
