"""Child process of tests/test_gpu_encode.py::test_phase_splits_in_a_fresh_process.  The tiled encoder's phase split (DNS_ENC_PHASES =
"pe_ph,g_ph") is read once per process, so every setting needs a process of its own: this one runs the `edges` forward and d_x cases
of test_gpu_encode.py against the float64 reference under whatever the environment holds, prints one `REPORT <worst ratio> <case>`
line per case and `OK phases <setting>`, and exits non-zero on the first miss."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_gpu_encode as t  # noqa: E402


def main():
    out = []
    for grid in ("16_592", "14_128_L4"):
        for n_bins in (16, 12, 5):
            out.append((t.run_forward("edges", grid, n_bins, "joint"), f"fwd joint edges grid {grid} n_bins {n_bins}"))
            for saved in (True, False):
                out.append((t.run_dx("edges", grid, n_bins, "joint", saved), f"d_x joint {'saved' if saved else 'regather'} edges grid {grid} n_bins {n_bins}"))
        out.append((t.run_forward("world", grid, 16, "joint", "spread"), f"fwd joint world grid {grid} n_bins 16 spread"))
        out.append((t.run_dx("world", grid, 8, "joint", True, "spread", "spread"), f"d_x joint saved world grid {grid} n_bins 8 spread"))
    for n_bins in (16, 5):
        out.append((t.run_forward("edges", "16_592", n_bins, "pe"), f"fwd OneBlob alone edges n_bins {n_bins}"))
        out.append((t.run_dx("edges", "16_592", n_bins, "pe", True), f"d_x OneBlob alone edges n_bins {n_bins}"))
    for worst, what in out:
        print(f"REPORT {worst:.4f} {what}")
    print("OK phases " + os.environ.get("DNS_ENC_PHASES", "default"), flush=True)


if __name__ == "__main__":
    main()
