"""ops.ms_ssim (the fused launch sequence of csrc/image_metrics.hip, and the same definition composed from torch ops on the
device, method="torch") and ops.label_confusion on image pairs of 680 x 1200 and 480 x 640: ms per call and launches per call.

    python tools/time_image_metrics.py [--reps 20] [--frames 1] [--out profiles/image_metrics_time.txt]

Every measurement is a child process of its own under `timeout` (--step NAME --size HxW runs one of them in this process); the
first one that fails ends the run.  Launches: of the library's entry points, the kernel spans dns_kernel_timing records; of the
torch composition, the aten operators that are not views, each of which launches at least one kernel.
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ("680x1200", "480x640")
STEPS = ("ms_ssim_fused", "ms_ssim_torch", "confusion_lds", "confusion_global")
VIEWS = ("view", "permute", "expand", "reshape", "slice", "select", "unsqueeze", "squeeze", "detach", "alias", "transpose", "t",
         "as_strided", "unflatten", "flatten", "_unsafe_view", "lift_fresh")


def run_step(step, size, reps, frames):
    import torch
    if step == "device":
        print(torch.cuda.get_device_name())
        return
    from torch.utils._python_dispatch import TorchDispatchMode
    from dns_slam_amd import _lib, ops

    class Count(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if func.overloadpacket.__name__ not in VIEWS:
                Count.n += 1
            return func(*args, **(kwargs or {}))

    H, W = (int(v) for v in size.split("x"))
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    if step.startswith("ms_ssim"):
        gt = torch.rand(frames, H, W, 3, device=dev, generator=g)
        pred = (gt + 0.05 * torch.randn(frames, H, W, 3, device=dev, generator=g)).clamp(0, 1)
        depth = torch.rand(frames, H, W, device=dev, generator=g) - 0.02
        method = step.split("_")[-1]
        fn = lambda: ops.ms_ssim_launch(pred, gt, depth, method=method)
    else:
        nc = 40 if step == "confusion_lds" else ops.CONFUSION_LDS_CLASSES + 36
        a = torch.randint(0, nc, (frames, H, W), device=dev, generator=g, dtype=torch.int32)
        b = torch.where(torch.rand(frames, H, W, device=dev, generator=g) < 0.8, a,
                        torch.randint(0, nc, (frames, H, W), device=dev, generator=g, dtype=torch.int32))
        fn = lambda: ops.label_confusion(a, b, nc)
    for _ in range(3):
        out = fn()
    torch.cuda.synchronize()
    if step == "ms_ssim_torch":
        with Count():
            fn()
        launches = Count.n
    else:
        _lib.lib.dns_kernel_timing(1)
        k0 = _lib.lib.dns_kernel_timing_count()
        fn()
        torch.cuda.synchronize()
        launches = _lib.lib.dns_kernel_timing_count() - k0
        _lib.lib.dns_kernel_timing(0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = time.perf_counter()
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t) / reps * 1e3
    dev_ms = e0.elapsed_time(e1) / reps
    extra = f"ms_ssim[0] {float(out[0][0]):.6f}" if step.startswith("ms_ssim") else f"trace {int(out[0].diagonal(dim1=-2, dim2=-1).sum())}"
    print(f"  {step:17s} {size:9s} F={frames}  {dev_ms:9.4f} ms/call on the stream  {wall:9.4f} ms/call wall  {launches:4d} launches   ({extra})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=1)
    ap.add_argument("--step", choices=STEPS + ("device",))
    ap.add_argument("--size", default=SIZES[0])
    ap.add_argument("--limit", type=int, default=120, help="seconds per measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_metrics_time.txt"))
    a = ap.parse_args()
    if a.step:
        run_step(a.step, a.size, a.reps, a.frames)
        return
    # this process never touches the GPU: every measurement, the device's name included, is a fresh child
    print(f"ops.ms_ssim / ops.label_confusion, {a.reps} calls each after 3 warm-up calls; device:", flush=True)
    lines = [f"ops.ms_ssim / ops.label_confusion, {a.reps} calls each after 3 warm-up calls",
             "  (stream: events round the calls; wall: host time per call including the allocations and the final synchronise)"]
    for size, step in [(SIZES[0], "device")] + [(size, step) for size in SIZES for step in STEPS]:
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step", step, "--size",
                            size, "--reps", str(a.reps), "--frames", str(a.frames)], capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            print(f"  {step} {size}: exit status {r.returncode}; stopping here")
            sys.exit(1)
        lines += [l for l in r.stdout.splitlines() if l.strip()]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
