"""Generate tests/golden/phi4_metropolis.json: <phi^2> of the interacting phi^4 lattice under exp(-S / C^2)
from a sampler that shares nothing with the library's Langevin, MALA or HMC code.

Run:  python tests/golden/make_phi4_metropolis.py          (about a quarter of an hour)
Pure NumPy float64; does not touch the library, the oracle or the reference.

The action is include/stochquant.h's, on the periodic Lx x Ly x Lz lattice:

    S = sum_x [ (3 + m2 / 2) phi_x^2 + (lam / 24) phi_x^4 - sum_mu phi_x phi_{x + mu} ]

so the part of S that holds one site's value f, its six neighbours summing to nb, is
s(f) = (3 + m2 / 2) f^2 + (lam / 24) f^4 - f nb.  One sweep is a Metropolis update of every even site
((x + y + z) even; their neighbours are all odd, so the updates are independent) and then of every odd site:
f' = f + WIDTH C (2 U - 1), accepted when U' < exp(-(s(f') - s(f)) / C^2).  Many independent chains run
side by side; the observable is <phi^2> = mean over sites, sweeps and chains of phi^2, its standard error the
spread of the chain means over sqrt(chains), which no autocorrelation within a chain can flatter.
"""
import json
import os

import numpy as np

SHAPE = (8, 4, 4)              # Lx, Ly, Lz: all even, so the checkerboard closes periodically
POINT = dict(m2=0.25, lam=6.0, C=0.7)
THERM, SEED = 200, 20241
# (parameters, chains, sweeps) per entry.  The target's size makes its standard error, 1.6e-5, a third of the
# smaller of the two GPU runs' (HMC: 5.0e-5); the other two values only have to be told apart from it.
RUNS = {"target": (POINT, 4096, 3200), "free": (dict(POINT, lam=0.0), 2048, 2400),
        "unit_noise": (dict(POINT, C=1.0), 2048, 2400)}
WIDTH = 1.7                    # proposal half-width over C: some 0.36 of the proposals are accepted


def sample(m2, lam, C, chains, sweeps, therm, seed, shape=SHAPE):
    """(mean, standard error, acceptance) of <phi^2> over `sweeps` sweeps after `therm` dropped ones."""
    Lx, Ly, Lz = shape
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(Lz), np.arange(Ly), np.arange(Lx), indexing="ij")
    masks = [((x + y + z) % 2 == p) for p in (0, 1)]
    km, l24, c2 = 3.0 + 0.5 * m2, lam / 24.0, C * C
    phi = 0.3 * C * rng.standard_normal((chains, Lz, Ly, Lx))
    tot = np.zeros(chains)
    acc = n = 0
    for sweep in range(therm + sweeps):
        for mask in masks:
            nb = sum(np.roll(phi, d, axis=a) for a in (1, 2, 3) for d in (1, -1))[:, mask]
            f = phi[:, mask]
            g = f + WIDTH * C * (2.0 * rng.random(f.shape) - 1.0)
            ds = km * (g * g - f * f) + l24 * (g ** 4 - f ** 4) - (g - f) * nb
            ok = rng.random(f.shape) < np.exp(np.minimum(-ds / c2, 0.0))
            phi[:, mask] = np.where(ok, g, f)
            if sweep >= therm:
                acc += int(ok.sum())
                n += ok.size
        if sweep >= therm:
            tot += (phi * phi).mean(axis=(1, 2, 3))
    per = tot / sweeps
    return float(per.mean()), float(per.std(ddof=1) / np.sqrt(chains)), acc / n


def main():
    out = {"shape": list(SHAPE), "therm": THERM, "seed": SEED, "width": WIDTH}
    for k, (name, (par, chains, sweeps)) in enumerate(RUNS.items()):
        mean, sem, acc = sample(par["m2"], par["lam"], par["C"], chains, sweeps, THERM, SEED + k)
        out[name] = {"m2": par["m2"], "lam": par["lam"], "C": par["C"], "chains": chains, "sweeps": sweeps,
                     "phi2": mean, "sem": sem, "acceptance": acc}
        print(name, out[name], flush=True)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "phi4_metropolis.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
