"""Largest connected component per case: the host route (test_util.getLargestCC, scipy) against the GPU route (csrc/cc.hip,
utils/cc_gpu.py), and what the device-resident tail of eval_surface.test_all_case(cc="gpu") is worth per case.

Inputs at 112x112x80 (the LA patch) and 192x160x88 (an LA-sized whole case): a ball plus 0.2 % speckle (what a prediction looks like:
one big component and debris), and 30 % random density (many components, the union pass at work).  Per input:
  host        getLargestCC on the numpy array                                                        (time.perf_counter)
  gpu kernels cc_gpu.components between two device events (memset + the five passes)
  gpu wall    cc_gpu.largest_cc on a label volume that is on the device (what predict_case leaves): kernels, the copy of `info`
  gpu wall+up the same from the numpy array: the upload of one byte per voxel included
and per shape the time per case of eval_surface.test_all_case(nms=1, surface="gpu") with cc="host" against cc="gpu" on the package's
V-Net (16 filters, eval mode, random weights; the input is the ball with noise; if the random network predicts no foreground its two
output channels are exchanged).  Medians.  largest_cc is compared with getLargestCC (array_equal) before anything is timed, and the
two evaluation routes with each other (dice, jc, hd95 ==, asd to 1e-12).

Every step runs in a child process of its own under --step-timeout seconds; the first step that fails or runs out of time ends the
run (nothing more is started on the GPU after it).

--by_value measures the by-value kernels (csrc/cc.hip) instead: label maps of 3 / 3 / 4 / 9 classes (--classes: that many for every
volume) at 112x112x80, 192x160x88 and twice 10x256x256 - one ball per class with 0.2 % speckle of random classes, and 30 % random
density.  Per input the host route cc_host.keep_largest_per_class, cc_gpu.components_by_value and the binary cc_gpu.components on the
same map's `!= 0` between device events, largest_per_class on a device tensor and from the numpy array, and largest_cc from the
numpy array of `!= 0` (what the value tests cost beside the binary route); the GPU routes are measured in turn, one call each per round.
Then one 2-D case (10 slices of 256 x 256, 4 classes, the package's U-Net with random weights) through
eval_surface.test_single_volume(nms=1, surface="gpu", zoom="gpu") with cc="host" against cc="gpu".

  python tools/cc_bench.py [--by_value [--classes C]] [--reps 10 --warmup 3 --host-reps 5 --eval-reps 3 --step-timeout 300]
                           [--out cc_bench_table.md]
--out writes the tables and the line under them, nothing else.  profiles/cc_gpu_notes.md quotes such tables inside notes written by
hand; the tool refuses to overwrite that file."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SHAPES = {"112x112x80": (112, 112, 80), "192x160x88": (192, 160, 88)}
INPUTS = ("ball + 0.2 % speckle", "30 % random")
TAG = "CC_BENCH "


def ball(shape, radius_frac=0.35):
    g = np.indices(shape).astype(np.float64)
    return sum((g[i] - shape[i] / 2) ** 2 for i in range(len(shape))) < (radius_frac * min(shape)) ** 2


def make_input(shape, kind):
    rng = np.random.default_rng(sum(shape))
    if kind == INPUTS[0]:
        return (ball(shape) | (rng.random(shape) < 0.002)).astype(np.int64)
    return (rng.random(shape) < 0.3).astype(np.int64)


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown CPU"


# ---- the steps (each in a child process) ------------------------------------------------------------------------------------------------
def step_cc(shape_name, kind, args):
    import torch
    from arco_amd.test_util import getLargestCC
    from arco_amd.utils import cc_gpu
    x = make_input(SHAPES[shape_name], kind)
    xd = torch.from_numpy(x).cuda()
    host = getLargestCC(x)
    assert np.array_equal(cc_gpu.largest_cc(xd).cpu().numpy(), host) and np.array_equal(cc_gpu.largest_cc(x).cpu().numpy(), host)
    info = cc_gpu.components(xd)[2].cpu().tolist()
    t_host = median_ms(lambda: getLargestCC(x), args.host_reps, 1)
    ts = []
    for i in range(args.warmup + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        cc_gpu.components(xd)
        e1.record()
        e1.synchronize()
        if i >= args.warmup:
            ts.append(e0.elapsed_time(e1))
    t_wall = median_ms(lambda: cc_gpu.largest_cc(xd), args.reps, args.warmup)
    t_up = median_ms(lambda: cc_gpu.largest_cc(x), args.reps, args.warmup)
    return dict(shape=shape_name, kind=kind, components=info[0], largest=info[2], host=t_host, kernels=statistics.median(ts), wall=t_wall,
                up=t_up, gpu=torch.cuda.get_device_name(0))


def step_eval(shape_name, args):
    import torch
    from arco_amd import eval_surface
    from arco_amd.networks.vnetWithArgs import VNet
    shape = SHAPES[shape_name]
    rng = np.random.default_rng(7)
    label = ball(shape).astype(np.int64)
    image = (label + 0.5 * rng.standard_normal(shape)).astype(np.float32)
    torch.manual_seed(0)
    net = VNet(n_channels=1, n_classes=2, n_filters=16, normalization='batchnorm', has_dropout=False).cuda().eval()
    kw = dict(patch_size=(112, 112, 80), stride_xy=18, stride_z=4)
    swapped = False
    if not bool(eval_surface.predict_case(net, image, 18, 4, kw["patch_size"], 2).any()):
        inner = net

        class Swapped(torch.nn.Module):
            def forward(self, x):
                y = inner(x)
                return (y[0] if isinstance(y, (tuple, list)) else y).flip(1)
        net, swapped = Swapped().cuda().eval(), True
    cases = [(image, label)]
    out = {}
    for cc in ("host", "gpu"):
        out[cc] = eval_surface.test_all_case(net, cases, 2, nms=1, surface="gpu", cc=cc, **kw)
    h, g = out["host"], out["gpu"]
    assert np.array_equal(h[:3], g[:3]) and abs(g[3] - h[3]) <= 1e-12 * abs(h[3]), (h, g)
    res = dict(shape=shape_name, swapped=swapped, metrics=[float(v) for v in h])
    for cc in ("host", "gpu"):
        def run():
            eval_surface.test_all_case(net, cases, 2, nms=1, surface="gpu", cc=cc, **kw)
            torch.cuda.synchronize()
        res[cc] = median_ms(run, args.eval_reps, 1)
    return res


# ---- --by_value: components of equal values, the largest one of every class (csrc/cc.hip) ----------------------------------------
BV_VOLUMES = (("112x112x80", (112, 112, 80), 3), ("192x160x88", (192, 160, 88), 3), ("10x256x256", (10, 256, 256), 4),
              ("10x256x256", (10, 256, 256), 9))
BV_INPUTS = ("balls + 0.2 % speckle", "30 % random")


def make_input_by_value(shape, kind, classes):
    """Labels 0..classes-1: one ball per class side by side along the last axis with speckle of random classes, or 30 % random density."""
    rng = np.random.default_rng(sum(shape) + classes)
    values = rng.integers(1, classes, size=shape)
    if kind == BV_INPUTS[1]:
        return np.where(rng.random(shape) < 0.3, values, 0).astype(np.int64)
    g = np.indices(shape).astype(np.float64)
    x = np.zeros(shape, dtype=np.int64)
    step = shape[-1] / (classes - 1)
    semi = [0.45 * s for s in shape[:-1]] + [0.45 * step]           # (ellipsoids: the 2-D stacks are thin)
    for c in range(1, classes):
        centre = [s / 2 for s in shape[:-1]] + [(c - 0.5) * step]
        x[sum(((g[i] - centre[i]) / semi[i]) ** 2 for i in range(len(shape))) < 1.0] = c
    return np.where(rng.random(shape) < 0.002, values, x).astype(np.int64)


def step_by_value(index, kind, args):
    import torch
    from arco_amd.utils.cc_host import keep_largest_per_class
    from arco_amd.utils import cc_gpu
    name, shape, classes = BV_VOLUMES[index]
    classes = args.classes or classes
    x = make_input_by_value(shape, kind, classes)
    xd = torch.from_numpy(x).cuda()
    fg = x != 0
    host = keep_largest_per_class(x)
    assert np.array_equal(cc_gpu.largest_per_class(xd, classes).cpu().numpy(), host)
    assert np.array_equal(cc_gpu.largest_per_class(x, classes).cpu().numpy(), host)
    info = cc_gpu.components_by_value(xd, classes)[2].cpu().tolist()
    t_host = median_ms(lambda: keep_largest_per_class(x), args.host_reps, 1)

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    fd = torch.from_numpy(fg.astype(np.uint8)).cuda()
    routes = {                                                       # measured in turn, one call of each per round
        "kernels": lambda: events(lambda: cc_gpu.components_by_value(xd, classes)),
        "kernels_bin": lambda: events(lambda: cc_gpu.components(fd)),
        "wall": lambda: wall(lambda: cc_gpu.largest_per_class(xd, classes)),
        "up": lambda: wall(lambda: cc_gpu.largest_per_class(x, classes)),
        "up_bin": lambda: wall(lambda: cc_gpu.largest_cc(fg)),
    }
    ts = {k: [] for k in routes}
    for i in range(args.warmup + args.reps):
        for k, fn in routes.items():
            t = fn()
            if i >= args.warmup:
                ts[k].append(t)
    res = {k: statistics.median(v) for k, v in ts.items()}
    res.update(shape=name, kind=kind, classes=classes, components=info[0][0], host=t_host, gpu=torch.cuda.get_device_name(0))
    return res


def step_eval2d(args):
    """One 2-D case (10 slices of 256 x 256, 4 classes) through test_single_volume(nms=1, surface="gpu", zoom="gpu")."""
    import torch
    from arco_amd import eval_surface
    from arco_amd.networks.unetWithArgs import UNet
    C, shape = args.classes or 4, (10, 256, 256)
    rng = np.random.default_rng(11)
    label = make_input_by_value(shape, BV_INPUTS[0], C)
    image = (label / C + 0.5 * rng.standard_normal(shape)).astype(np.float32)
    torch.manual_seed(0)
    net = UNet(in_chns=1, class_num=C).cuda().eval()
    kw = dict(surface="gpu", zoom="gpu", nms=1)
    out = {cc: eval_surface.test_single_volume(image, label, net, C, cc=cc, **kw) for cc in ("host", "gpu")}
    for h, g in zip(out["host"], out["gpu"]):
        assert h[:3] == g[:3] and abs(g[3] - h[3]) <= 1e-12 * abs(h[3]), (h, g)
    ts = {"host": [], "gpu": []}
    for i in range(1 + args.eval_reps):
        for cc in ("host", "gpu"):                                   # in turn
            t0 = time.perf_counter()
            eval_surface.test_single_volume(image, label, net, C, cc=cc, **kw)
            torch.cuda.synchronize()
            if i >= 1:
                ts[cc].append((time.perf_counter() - t0) * 1e3)
    return dict(shape="10x256x256", classes=C, host=statistics.median(ts["host"]), gpu=statistics.median(ts["gpu"]),
                metrics=[[float(v) for v in m] for m in out["host"]])


def main_by_value(args):
    rows, ev = [], None
    names = ["bv|%d|%s" % (i, k) for i in range(len(BV_VOLUMES)) for k in BV_INPUTS] + ["eval2d"]
    for name in names:
        cmd = [sys.executable, os.path.abspath(__file__), "--by_value", "--step", name, "--reps", str(args.reps), "--warmup", str(args.warmup),
               "--host-reps", str(args.host_reps), "--eval-reps", str(args.eval_reps)] + (["--classes", str(args.classes)] if args.classes else [])
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired as e:
            print(e.stdout or "")
            raise SystemExit("cc_bench: step %r ran past %.0f s; nothing more is started" % (name, args.step_timeout))
        found = [json.loads(l[len(TAG):]) for l in p.stdout.splitlines() if l.startswith(TAG)]
        if p.returncode != 0 or len(found) != 1:
            print(p.stdout)
            raise SystemExit("cc_bench: step %r failed with exit status %d; nothing more is started" % (name, p.returncode))
        if name == "eval2d":
            ev = found[0]
        else:
            rows.append(found[0])
        print(name, json.dumps(found[0]), flush=True)
    lines = ["| Volume | classes | input | components | host keep_largest_per_class | GPU kernels by value | GPU kernels binary | "
             "by value: wall (labels on the device) | by value: wall + upload | binary: wall + upload | host / by value + upload |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %d | %s | %d | %.1f ms | %.3f ms | %.3f ms | %.2f ms | %.2f ms | %.2f ms | %.1fx |" %
                     (r["shape"], r["classes"], r["kind"], r["components"], r["host"], r["kernels"], r["kernels_bin"], r["wall"], r["up"],
                      r["up_bin"], r["host"] / r["up"]))
    lines += ["", "| Volume | classes | test_single_volume(nms=1) per case, cc=\"host\" | cc=\"gpu\" | difference |", "|---|---|---|---|---|"]
    lines.append("| %s | %d | %.1f ms | %.1f ms | %.1f ms |" % (ev["shape"], ev["classes"], ev["host"], ev["gpu"], ev["host"] - ev["gpu"]))
    note = ("Host CPU: %s; GPU: %s.  Medians: host %d runs after 1, GPU %d rounds after %d with the routes measured in turn, "
            "test_single_volume %d rounds after 1 (surface=\"gpu\", zoom=\"gpu\", U-Net, random weights).  largest_per_class equals "
            "keep_largest_per_class (array_equal) at every input; cc=\"gpu\" equals cc=\"host\" (dice, jc, hd95 ==, asd within 1e-12)." %
            (cpu_model(), rows[0]["gpu"], args.host_reps, args.reps, args.warmup, args.eval_reps))
    table = "\n".join(lines)
    print(table + "\n\n" + note)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n\n" + note + "\n")


def steps():
    for s in SHAPES:
        for k in INPUTS:
            yield "cc|%s|%s" % (s, k)
    for s in SHAPES:
        yield "eval|%s" % s


def run_step(name, args):
    parts = name.split("|")
    if parts[0] in ("bv", "eval2d"):
        res = step_by_value(int(parts[1]), parts[2], args) if parts[0] == "bv" else step_eval2d(args)
        print(TAG + json.dumps(res), flush=True)
        return
    res = step_cc(parts[1], parts[2], args) if parts[0] == "cc" else step_eval(parts[1], args)
    print(TAG + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--eval-reps", type=int, default=3)
    ap.add_argument("--step-timeout", type=float, default=300.0, help="seconds for each step (a child process of its own)")
    ap.add_argument("--out", default=None, help="also write the tables to this file (not profiles/cc_gpu_notes.md)")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--by_value", action="store_true", help="the by-value tables (the ccv_* kernels of cc.hip: components of equal values, per-class winners)")
    ap.add_argument("--classes", type=int, default=None, help="with --by_value: this class count (2..256) for every volume instead of 3 / 3 / 4 / 9")
    args = ap.parse_args()
    if args.classes is not None and not (args.by_value and 2 <= args.classes <= 256):
        raise SystemExit("cc_bench: --classes goes with --by_value and lies in 2..256")
    if args.step:
        return run_step(args.step, args)
    if args.out and os.path.basename(args.out) == "cc_gpu_notes.md":
        raise SystemExit("cc_bench: profiles/cc_gpu_notes.md is written by hand around the tables of this tool; give --out another file")
    if args.by_value:
        return main_by_value(args)
    cc_rows, eval_rows = [], []
    for name in steps():
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps), "--warmup", str(args.warmup),
               "--host-reps", str(args.host_reps), "--eval-reps", str(args.eval_reps)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired as e:
            print(e.stdout or "")
            raise SystemExit("cc_bench: step %r ran past %.0f s; nothing more is started" % (name, args.step_timeout))
        found = [json.loads(l[len(TAG):]) for l in p.stdout.splitlines() if l.startswith(TAG)]
        if p.returncode != 0 or len(found) != 1:
            print(p.stdout)
            raise SystemExit("cc_bench: step %r failed with exit status %d; nothing more is started" % (name, p.returncode))
        r = found[0]
        if name.startswith("cc"):
            cc_rows.append(r)
            print("%-10s %-22s host %8.1f ms | gpu kernels %7.3f ms, wall %7.2f ms, wall + upload %7.2f ms | x%.1f" %
                  (r["shape"], r["kind"], r["host"], r["kernels"], r["wall"], r["up"], r["host"] / r["up"]), flush=True)
        else:
            eval_rows.append(r)
            print("%-10s test_all_case per case: cc=host %9.1f ms, cc=gpu %9.1f ms" % (r["shape"], r["host"], r["gpu"]), flush=True)
    lines = ["| Volume | input | components | host getLargestCC | GPU kernels | GPU wall (labels on the device) | GPU wall + upload | host / GPU wall + upload |",
             "|---|---|---|---|---|---|---|---|"]
    for r in cc_rows:
        lines.append("| %s | %s | %d | %.1f ms | %.3f ms | %.2f ms | %.2f ms | %.1fx |" %
                     (r["shape"], r["kind"], r["components"], r["host"], r["kernels"], r["wall"], r["up"], r["host"] / r["up"]))
    lines += ["", "| Volume | test_all_case per case, cc=\"host\" | cc=\"gpu\" | difference |", "|---|---|---|---|"]
    for r in eval_rows:
        lines.append("| %s | %.1f ms | %.1f ms | %.1f ms |" % (r["shape"], r["host"], r["gpu"], r["host"] - r["gpu"]))
    table = "\n".join(lines)
    note = ("Host CPU: %s; GPU: %s.  Medians: host %d runs after 1, GPU %d runs after %d, test_all_case %d runs after 1 "
            "(nms=1, surface=\"gpu\", V-Net 16 filters, patch 112x112x80, strides 18 / 4).  largest_cc equals getLargestCC (array_equal) "
            "at every input; cc=\"gpu\" equals cc=\"host\" (dice, jc, hd95 ==, asd within 1e-12): %s." %
            (cpu_model(), cc_rows[0]["gpu"], args.host_reps, args.reps, args.warmup, args.eval_reps,
             "; ".join("%s %s%s" % (r["shape"], ["%.4f" % v for v in r["metrics"]], " (channels exchanged)" if r["swapped"] else "")
                       for r in eval_rows)))
    print(table + "\n\n" + note)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n\n" + note + "\n")


if __name__ == "__main__":
    main()
