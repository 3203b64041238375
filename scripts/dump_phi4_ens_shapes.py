"""Every answer of the phi^4 ensemble's *_shape_info entry points, for every legal
lattice shape, one line per shape (CPU only; SQ_LIB=<path> selects the library).
Two libraries give the same launches exactly when their dumps are equal:

    python scripts/dump_phi4_ens_shapes.py | sha256sum
    python scripts/dump_phi4_ens_shapes.py --count      # shapes and hash only

Where a call refuses the shape, the line holds the refusal.
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stochquant_amd import Phi4Ensemble, StochQuantError  # noqa: E402

CALLS = ("shape_info", "corr_shape_info", "pcorr_shape_info", "flow_shape_info", "frames_flow_shape_info",
         "heun_frames_shape_info", "exchange_shape_info", "cluster_shape_info", "cluster_improved_shape_info")


def lines():
    for Lx in (8, 16, 32, 64):
        for Ly in range(2, 32768 // (2 * Lx) + 1):
            for Lz in range(2, 32768 // (Lx * Ly) + 1):
                row = [f"{Lx}x{Ly}x{Lz}"]
                for call in CALLS:
                    try:
                        d = getattr(Phi4Ensemble, call)((Lx, Ly, Lz))
                        row.append(call + ":" + ",".join(f"{k}={v}" for k, v in d.items()))
                    except StochQuantError as e:
                        row.append(f"{call}:refused({e.code}) {e}")
                yield " ".join(row)


def main():
    count = "--count" in sys.argv[1:]
    h, n = hashlib.sha256(), 0
    for line in lines():
        h.update((line + "\n").encode())
        n += 1
        if not count:
            print(line)
    if count:
        print(f"shapes={n} sha256={h.hexdigest()}")


if __name__ == "__main__":
    main()
