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

  python tools/cc_bench.py [--reps 10 --warmup 3 --host-reps 5 --eval-reps 3 --step-timeout 300] [--out cc_bench_table.md]
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


def steps():
    for s in SHAPES:
        for k in INPUTS:
            yield "cc|%s|%s" % (s, k)
    for s in SHAPES:
        yield "eval|%s" % s


def run_step(name, args):
    parts = name.split("|")
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
    args = ap.parse_args()
    if args.step:
        return run_step(args.step, args)
    if args.out and os.path.basename(args.out) == "cc_gpu_notes.md":
        raise SystemExit("cc_bench: profiles/cc_gpu_notes.md is written by hand around the tables of this tool; give --out another file")
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
