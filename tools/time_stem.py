"""Time the image stem: the HIP path (ops.stem_forward through encoder.ResNet(backend="hip")) against the stock composition
(ResNet(backend="torch") + the channels-last copy its consumers need, common.features_channels_last's expression), in both
normalisation modes, at the two dataset shapes -- Replica 12 x 680 x 1200 and ScanNet 12 x 460 x 620 (one optimize(): 4 target frames
x 3 reference views).

    python tools/time_stem.py [--reps 20] [--out stem_time.json]

Per path and mode: time per call and per image (device events around `reps` calls after warm-up, alternating the paths), the bytes
and operations the algorithm needs over that time -- 12 H W + 256 h w bytes (read the image, write the map once) and 2 * 147 * 64
flop per output pixel -- against the two floors (HBM at 4.5 TB/s, fp32 matrix pipe at 155 TFLOP/s), and the peak device memory of
one call above what the inputs hold.  In batch mode both ways to apply the statistics are timed: normalising the stored raw
convolution in place, and running the convolution a second time.  Outputs of the two paths are compared at the timed sizes.
The first stock call (library kernel search) is reported separately."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dns_slam_amd import ops                                   # noqa: E402
from dns_slam_amd.encoder import ResNet                        # noqa: E402

DEV = "cuda:0"
HBM_BPS, MATRIX_FLOPS = 4.5e12, 155e12
SHAPES = {"replica": (12, 680, 1200), "scannet": (12, 460, 620)}


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_stem.py measures on the GPU; none found")
    results = []
    for name, (n, H, W) in SHAPES.items():
        h, w = ops.stem_out_shape(H, W)
        nbytes, flop = n * (12 * H * W + 256 * h * w), n * h * w * 2 * 147 * 64
        floor_hbm, floor_mat = nbytes / HBM_BPS, flop / MATRIX_FLOPS
        images = torch.rand(1, n, H, W, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
        for bn in ("frozen", "batch"):
            hip, stock = ResNet(seed=3, backend="hip", bn=bn).to(DEV), ResNet(seed=3, backend="torch", bn=bn).to(DEV)
            st = hip.conv_blocks
            par = (st.conv1.weight, st.bn1.weight, st.bn1.bias, st.bn1.running_mean, st.bn1.running_var)
            flat = images[0]
            paths = {"hip": lambda: hip(images),
                     "stock+nhwc": lambda: stock(images)[0].permute(0, 2, 3, 1).contiguous()}
            if bn == "batch":
                paths["hip-recompute"] = lambda: ops.stem_forward(flat, *par, batch_stats=True, batch_apply="recompute")
            t0 = time.perf_counter()
            ref = paths["stock+nhwc"]()
            torch.cuda.synchronize()
            first_stock = time.perf_counter() - t0
            got = hip(images)[0].permute(0, 2, 3, 1)
            diff = float((got - ref).abs().max() / ref.abs().max())
            del ref, got
            for fn in paths.values():                              # warm-up of every shape and path
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in paths}
            for _ in range(3):                                     # alternate the paths: three windows each
                for k, fn in paths.items():
                    times[k].append(timed(fn, a.reps))
            for k, fn in paths.items():
                t = sorted(times[k])[1]
                row = {"shape": name, "n": n, "H": H, "W": W, "bn": bn, "path": k, "ms_per_call": t * 1e3, "us_per_image": t / n * 1e6,
                       "ms_windows": [x * 1e3 for x in times[k]], "GBps": nbytes / t * 1e-9, "TFLOPs": flop / t * 1e-12,
                       "floor_hbm_us_per_image": floor_hbm / n * 1e6, "floor_matrix_us_per_image": floor_mat / n * 1e6,
                       "share_of_floor": max(floor_hbm, floor_mat) / t, "peak_MB": peak_above_inputs(fn) / 1e6,
                       "max_rel_diff_vs_stock": diff}
                if k == "stock+nhwc":
                    row["first_call_s"] = first_stock
                results.append(row)
                print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
