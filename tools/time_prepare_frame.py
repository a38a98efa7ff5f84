"""Frame preparation (csrc/frame_prep.hip, ops.prepare_frames) at the datasets' sizes: Replica 680 x 1200 (every stage the identity)
and ScanNet 968 x 1296 -> 480 x 640 with crop_edge 10, for one frame and for 8 frames.

    python tools/time_prepare_frame.py [--reps 20] [--cpu-reps 3] [--out profiles/prepare_frame_time.txt]

Device lines: the kernel (one launch) against ``method="torch"`` (the same definition composed of torch ops on the device), called in
turn and timed with device events after 3 warm-up rounds: median and min .. max of ``--reps`` repetitions.  Bytes moved are the
compulsory ones of the shapes (every raw input byte once, every output byte once); the rate they give is set against the HBM copy
ceiling ``tools/stream_rate`` measures on the same device (built from tools/stream_rate.hip; without the binary no ceiling is printed).
``ops.label_first_seen`` on one label image is timed the same way.

CPU line: the reference's host procedure for ONE frame restated in numpy -- ``np.vectorize`` over a dict for every label pixel
included, cv2's two resizes as the table gathers of the published rules -- followed by the three host-to-device copies of the float
images, wall time, median and min .. max of ``--cpu-reps`` repetitions.  File decoding is in neither line.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# name -> (colour, depth, labels, label dtype, crop_size, crop_edge, png_depth_scale, distinct labels)
SHAPES = {"replica": ((680, 1200), (680, 1200), (680, 1200), np.uint8, None, 0, 6553.5, 40),
          "scannet": ((968, 1296), (480, 640), (968, 1296), np.uint16, None, 10, 1000.0, 30)}


def alternate(fns, reps, warm=3):
    """ms per call of every function, called in turn: [(median, min, max)]"""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ev = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    out = []
    for pairs in ev:
        t = [a.elapsed_time(b) for a, b in pairs]
        out.append((statistics.median(t), min(t), max(t)))
    return out


def copy_ceiling():
    """TB/s of the best float4 copy of tools/stream_rate, or None without the binary."""
    exe = os.path.join(ROOT, "tools", "stream_rate")
    if not os.path.exists(exe):
        return None
    r = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    rates = [float(m) for m in re.findall(r"copy4.*?([0-9.]+) TB/s", r.stdout)]
    return max(rates) if r.returncode == 0 and rates else None


def raw_frames(name, n, seed=0):
    chw, dhw, lhw, ldt, _, _, _, n_lab = SHAPES[name]
    g = np.random.default_rng(seed)
    color = g.integers(0, 256, size=(n,) + chw + (3,), dtype=np.uint8)
    depth = g.integers(0, 65536, size=(n,) + dhw).astype(np.uint16)
    # label images of large constant regions, as rendered semantics are: blocks of 40 x 40 pixels
    values = g.choice(256 if ldt == np.uint8 else 1200, size=n_lab, replace=False)
    blocks = values[g.integers(0, n_lab, size=(n, (lhw[0] + 39) // 40, (lhw[1] + 39) // 40))]
    label = np.repeat(np.repeat(blocks, 40, 1), 40, 2)[:, :lhw[0], :lhw[1]].astype(ldt)
    return color, depth, np.ascontiguousarray(label), values


def host_reference(color, depth, label, l2c, name, dev):
    """BaseDataset.__getitem__ for one frame, on the host, then the copies"""
    import frame_prep_ref as fr
    chw, dhw, lhw, _, crop_size, edge, pds, _ = SHAPES[name]
    v_map = np.vectorize(lambda value: l2c.get(value, value))
    c = color[..., ::-1].astype(np.float32) / 255.              # cv2.cvtColor(BGR2RGB), then the float conversion
    d = depth.astype(np.float32) / pds
    if chw != dhw:                                             # cv2.resize(color_data, (W, H)), in fp32
        (ix, wx), (iy, wy) = fr.cv_linear_table(chw[1], dhw[1]), fr.cv_linear_table(chw[0], dhw[0])
        h = c[:, ix] * wx[None, :, 0, None] + c[:, np.minimum(ix + 1, chw[1] - 1)] * wx[None, :, 1, None]
        c = h[iy] * wy[:, 0, None, None] + h[np.minimum(iy + 1, chw[0] - 1)] * wy[:, 1, None, None]
    lab = label.astype(np.float32)
    if lhw != dhw:
        lab = lab[fr.cv_nearest_table(lhw[0], dhw[0])][:, fr.cv_nearest_table(lhw[1], dhw[1])]
    lab = v_map(lab)
    c, d, lab = torch.from_numpy(c), torch.from_numpy(d) * 1.0, torch.from_numpy(lab)
    if edge > 0:
        c, d, lab = c[edge:-edge, edge:-edge], d[edge:-edge, edge:-edge], lab[edge:-edge, edge:-edge]
    out = c.to(dev), d.to(dev), lab.to(dev)
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prepare_frame_time.txt"))
    a = ap.parse_args()
    ceiling = copy_ceiling()                                   # a child process, before this one opens the device
    from dns_slam_amd import ops
    dev = "cuda:0"
    lines = [f"ops.prepare_frames on {torch.cuda.get_device_name()}: device events, 3 warm-up + {a.reps} alternating repetitions, median (min .. max)",
             "HBM copy ceiling (tools/stream_rate, best float4 copy): " + (f"{ceiling:.2f} TB/s" if ceiling else "not measured (no tools/stream_rate binary)")]
    print("\n".join(lines), flush=True)

    def say(s):
        lines.append(s)
        print(s, flush=True)

    for name, (chw, dhw, lhw, ldt, crop_size, edge, pds, _) in SHAPES.items():
        tables = ops.frame_prep_tables(chw, dhw, lhw, crop_size, edge, dev)
        for n in (1, 8):
            color, depth, label, values = raw_frames(name, n)
            l2c = {int(v): k for k, v in enumerate(values)}
            lut = torch.tensor([l2c.get(v, v) for v in range(ops.LABEL_VALUES)], dtype=torch.int32, device=dev)
            c, d, l = (torch.from_numpy(x).to(dev) for x in (color, depth, label))
            fns = [lambda m=m: ops.prepare_frames(c, d, l, lut, tables, pds, 1.0, bgr=True, method=m) for m in ("kernel", "torch")]
            kc, kd, kl = fns[0]()
            tc, td, tl = fns[1]()
            same = f"depth {'equal' if torch.equal(kd, td) else 'DIFFERS'}, label {'equal' if torch.equal(kl, tl) else 'DIFFERS'}, colour max |kernel - torch| {float((kc - tc).abs().max()):.2e}"
            (km, k0, k1), (tm, t0, t1) = alternate(fns, a.reps)
            moved = c.numel() + 2 * d.numel() + l.numel() * l.element_size() + 4 * (kc.numel() + kd.numel()) + 8 * kl.numel()
            rate = moved / (km * 1e-3) / 1e12
            frac = f" = {100 * rate / ceiling:.0f} % of the copy ceiling" if ceiling else ""
            say(f"{name:8s} n={n}  {chw[0]} x {chw[1]} -> {tables.H} x {tables.W}   kernel {km:.4f} ms ({k0:.4f} .. {k1:.4f})   torch {tm:.4f} ms ({t0:.4f} .. {t1:.4f})"
                f"   {moved / 1e6:.1f} MB moved, {rate:.3f} TB/s{frac}   [{same}]")
            if n == 1:
                (fm, f0, f1), = alternate([lambda: ops.label_first_seen(l)], a.reps)
                say(f"{name:8s} label_first_seen on one {lhw[0]} x {lhw[1]} {np.dtype(ldt).name} image: {fm:.4f} ms ({f0:.4f} .. {f1:.4f})")
                host_reference(color[0], depth[0], label[0], l2c, name, dev)
                t = []
                for _ in range(a.cpu_reps):
                    t0_ = time.perf_counter()
                    hc, hd, hl = host_reference(color[0], depth[0], label[0], l2c, name, dev)
                    t.append((time.perf_counter() - t0_) * 1e3)
                ok = torch.equal(hl, kl[0]) and torch.equal(hd, kd[0])
                say(f"{name:8s} n=1  the reference's host procedure in numpy + 3 copies: {statistics.median(t):.1f} ms ({min(t):.1f} .. {max(t):.1f}) wall"
                    f"   [depth and label {'equal' if ok else 'DIFFER from'} the kernel's]")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
