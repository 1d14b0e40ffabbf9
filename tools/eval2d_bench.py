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

Every step runs in a child process of its own under --step-timeout seconds; the first step that fails or runs out of time ends the
run (nothing more is started on the GPU after it).

  python tools/eval2d_bench.py [--reps 10 --warmup 3 --kernel-reps 50 --step-timeout 300] [--out eval2d_bench_table.md]
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


def steps():
    for s in SHAPES:
        yield "case|%s" % s
    for s in SHAPES:
        yield "kernels|%s" % s


def run_step(name, args):
    kind, shape = name.split("|")
    res = step_case(shape, args) if kind == "case" else step_kernels(shape, args)
    print(TAG + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--step-timeout", type=float, default=300.0, help="seconds for each step (a child process of its own)")
    ap.add_argument("--out", default=None, help="also write the tables to this file (not profiles/eval2d_gpu_notes.md)")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return run_step(args.step, args)
    if args.out and os.path.basename(args.out) == "eval2d_gpu_notes.md":
        raise SystemExit("eval2d_bench: profiles/eval2d_gpu_notes.md is written by hand around the tables of this tool; give --out another file")
    case_rows, kernel_rows = [], []
    for name in steps():
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
        if name.startswith("case"):
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
    print(table + "\n\n" + note)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n\n" + note + "\n")


if __name__ == "__main__":
    main()
