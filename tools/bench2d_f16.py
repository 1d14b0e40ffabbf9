"""Same-process A/B of the 2-D step's activation storage: one stepper per mode (f32x3 default, --act_dtype f16, and f16rows =
--act_dtype f16 --fm_rows f16; own graphs and pack plans), alternating blocks of steps on the same batches on one box, after the warm-up the headline uses (graphs captured, then
--settle_steps untimed steps as bench.py runs them).  Prints one JSON line: ms/step per mode, the ratio, overflow_steps, final LOSS_SCALE.
python tools/bench2d_f16.py [--reps 8] [--block 100] [--settle_steps 240] [--only f16rows]      (--only: one mode, for a profiler run)"""
import argparse, json, os, sys, time
os.environ.setdefault("OMP_NUM_THREADS", "4")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from arco_amd import ops, train_arco_2d as T
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=8)
ap.add_argument("--block", type=int, default=100)
ap.add_argument("--settle_steps", type=int, default=240)
ap.add_argument("--only", type=str, default="", choices=["", "f32x3", "f16", "f16rows"])
a = ap.parse_args()
modes = [a.only] if a.only else ["f32x3", "f16", "f16rows"]
EXTRA = {"f32x3": [], "f16": ["--act_dtype", "f16"], "f16rows": ["--act_dtype", "f16", "--fm_rows", "f16"]}
base = ["--batch_size", "8", "--queue_size", "4096", "--func", "smc", "--synthetic", "1"]
sts, scale = {}, {}
for m in modes:
    args = T.build_parser().parse_args(base + EXTRA[m])
    sts[m] = T.ArcoStep2D(args, "cuda:0")
    scale[m] = ops.LOSS_SCALE
bs = [(T.synthetic_batch(8, args.patch_size, 4, 100 + 2 * i, "cuda:0"), T.synthetic_batch(8, args.patch_size, 4, 101 + 2 * i, "cuda:0")[0]) for i in range(4)]
def run(m, n):
    ops.ACT_HALF, ops.LOSS_SCALE = m != "f32x3", scale[m]        # process-wide switches: each stepper runs under its own
    st = sts[m]
    for i in range(n):
        (l, ll), u = bs[i % 4]
        st.step(l, ll, u, 0, 100)
    scale[m] = ops.LOSS_SCALE
for m in modes:
    run(m, 14)                                  # first-use costs and the graph captures
for i in range(0, a.settle_steps, 10):          # clock settling, as bench.py: untimed load before the timed region
    for m in modes:
        run(m, min(10, a.settle_steps - i) // len(modes) or 1)
res = {m: [] for m in modes}
for r in range(a.reps):
    for m in (modes if r % 2 == 0 else modes[::-1]):
        torch.cuda.synchronize(); t0 = time.perf_counter(); run(m, a.block); torch.cuda.synchronize()
        res[m].append((time.perf_counter() - t0) / a.block * 1e3)
out = {"tool": "bench2d_f16", "config": "2-D step, 8 + 8 images of 256x256, 4 classes, queue 4096, default schedule", "block": a.block,
       "reps": a.reps, "ms_per_step": {m: round(sum(v) / len(v), 4) for m, v in res.items()},
       "ms_per_step_min": {m: round(min(v), 4) for m, v in res.items()}, "blocks_ms": {m: [round(x, 3) for x in v] for m, v in res.items()}}
if "f16" in res and "f32x3" in res:
    out["f16_over_f32x3"] = round(out["ms_per_step"]["f16"] / out["ms_per_step"]["f32x3"], 4)
if "f16rows" in res and "f16" in res:
    out["f16rows_over_f16"] = round(out["ms_per_step"]["f16rows"] / out["ms_per_step"]["f16"], 4)
if "f16" in sts:
    out["overflow_steps"], out["final_loss_scale"] = sts["f16"].overflow_steps, scale["f16"]
if "f16rows" in sts:
    out["overflow_steps_f16rows"], out["final_loss_scale_f16rows"] = sts["f16rows"].overflow_steps, scale["f16rows"]
print(json.dumps(out))
