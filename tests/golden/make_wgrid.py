"""Regenerates tests/golden/wgrid/wgrid.npz and tests/golden/wgrid/dwgrid.npz (a folder of its own: conftest.golden_cases()
takes every .npz directly under tests/golden for an lnprob fixture).  Needs mpmath (1.3.0); the tests only read the .npz.

wgrid.npz:  w(x + i a) = exp(-z^2) erfc(-i z) at 40 digits, stored as float64 H = Re w and L = Im w.  The (a, x) values sit
on and beside every tier boundary of the device evaluation (rbvfit_amd/csrc/voigt_w_device.h).

dwgrid.npz: what the derivatives of the optical depth are built from, at 40 digits, stored as float64:
    H = Re w,    Hx = Re w',  w' = -2 z w + 2i/sqrt(pi),    G = Re (z w)',  (z w)' = w + z w'      (and L = Im w)
on a grid that adds the a of b = 0.05, 0.002, 1e-4 km/s on MgII (0.15, 3.6, 73) and 7-, and both neighbours of every |x| at
which dw_fast changes its series (8, 15, 36, 140, 600, 1e4), w_generic its method (6) and the CPU yardstick its rule (30).
a < 0 (the reflection branch of w_generic) is out of scope here: no line has it inside a prior box with b > 0.

The file also holds the scales the tolerances of Hx and G are relative to, so that every consumer uses the same ones:
    scale_G  = max(|G|,  0.01 |H| / (1 + x^2 + a^2)),        scale_Hx = max(|Hx|, 0.01 |H| / (1 + |z|)).
In the wings these are |G| and |Hx| themselves (|G| / |H| -> 3/x^2 there): a line off the spectrum contributes nothing but
wings, so a term's error is held against the term's own size.  The floors only cover the sign changes (G near x ~ 0.7 for
small a and near x ~ a/sqrt(3) for large a; Hx at x = 0), where neighbouring pixels of size ~|H|/|z|^2 carry the sum.
The assertions at the end keep the floors there: active on at most 5 % of the points, on none with |x| >= max(8, 2a)."""
import os

import mpmath
import numpy as np

mpmath.mp.dps = 40

A = np.array([0.0, 1e-6, 1e-3, 0.05, 0.1, np.nextafter(0.1, 1.0), 1.0, 7.0, 20.0])
XPOS = np.array([0.0, 1e-8, 1e-3, 0.1, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 2.5, 3.0, 3.7, 4.0, 4.99, 5.0, 5.5, 5.9, np.nextafter(6.0, 0.0), 6.0,
                 6.1, 7.0, 7.2, 7.49, 7.9, np.nextafter(8.0, 0.0), 8.0, np.nextafter(8.0, 9.0), 8.5, 9.0, 12.0, 14.0, 14.99, 15.0, 20.0,
                 30.0, 35.9, 36.0, 50.0, 100.0, 139.0, 140.0, 500.0, 599.0, 600.0, 3000.0, 9999.0, 1e4])
X = np.concatenate([-XPOS[:0:-1], XPOS])

DW_A = np.concatenate([A, [0.15, 3.6, np.nextafter(7.0, 0.0), 73.0]])
DW_EDGES = [8.0, 15.0, 36.0, 140.0, 600.0, 1e4]          # dw_fast: X_CORE and the boundaries of its shorter series
DW_XPOS = np.unique(np.concatenate([XPOS, [f(e, t) for e in DW_EDGES for f, t in ((np.nextafter, 0.0), (np.nextafter, np.inf))],
                                    DW_EDGES, [np.nextafter(6.0, 0.0), 6.0, 29.9, 30.0]]))
DW_X = np.concatenate([-DW_XPOS[:0:-1], DW_XPOS])


def w(x, a):
    z = mpmath.mpc(mpmath.mpf(float(x)), mpmath.mpf(float(a)))
    return mpmath.exp(-z * z) * mpmath.erfc(-1j * z)


def dw(x, a):
    """(w, w', (z w)') at 40 digits.  w' loses |z|^2 digits to cancellation (2 z w -> 2i/sqrt(pi)) and (z w)' twice that: the
    working precision is raised by 4 log10 |z| + 10 digits for the three of them."""
    z = mpmath.mpc(mpmath.mpf(float(x)), mpmath.mpf(float(a)))
    with mpmath.workdps(40 + 10 + int(4 * np.log10(1.0 + abs(complex(x, a))))):
        v = mpmath.exp(-z * z) * mpmath.erfc(-1j * z)
        d = -2 * z * v + 2j / mpmath.sqrt(mpmath.pi)
        return v, d, v + z * d


def scales(a, x, H, Hx, G):
    a, x = a[:, None], x[None, :]
    floor_G = 0.01 * np.abs(H) / (1.0 + x * x + a * a)
    floor_Hx = 0.01 * np.abs(H) / (1.0 + np.hypot(x, a))
    return np.maximum(np.abs(G), floor_G), np.maximum(np.abs(Hx), floor_Hx), np.abs(G) < floor_G, np.abs(Hx) < floor_Hx


def make_wgrid(folder):
    H = np.empty((A.size, X.size))
    L = np.empty((A.size, X.size))
    for i, a in enumerate(A):
        for j, x in enumerate(X):
            v = w(x, a)
            H[i, j] = float(v.real)
            L[i, j] = float(v.imag)
    out = os.path.join(folder, "wgrid.npz")
    np.savez_compressed(out, a=A, x=X, H=H, L=L)
    print(out, H.shape, os.path.getsize(out), "bytes")


def make_dwgrid(folder):
    H, L, Hx, G = (np.empty((DW_A.size, DW_X.size)) for _ in range(4))
    for i, a in enumerate(DW_A):
        for j, x in enumerate(DW_X):
            v, d, g = dw(x, a)
            H[i, j], L[i, j], Hx[i, j], G[i, j] = float(v.real), float(v.imag), float(d.real), float(g.real)
    sG, sHx, fG, fHx = scales(DW_A, DW_X, H, Hx, G)
    # a = 0: H = exp(-x^2) underflows beyond |x| ~ 27 and every scale with it; those points hold exact zeros
    live = H != 0.0
    far = np.abs(DW_X)[None, :] >= np.maximum(8.0, 2.0 * DW_A)[:, None]
    for name, f in (("G", fG), ("Hx", fHx), ("G or Hx", fG | fHx)):
        print("floor of %-7s active on %3d of %d points (%.2f %%), beyond max(8, 2a): %d"
              % (name, np.sum(f & live), live.sum(), 100.0 * np.sum(f & live) / live.sum(), np.sum(f & live & far)))
    assert np.sum((fG | fHx) & live) <= 0.05 * live.sum(), "the floors must stay an exception: change the grid, not the floor"
    assert not np.any((fG | fHx) & live & far), "no floor in the wings: a term's error is held against the term itself"
    out = os.path.join(folder, "dwgrid.npz")
    np.savez_compressed(out, a=DW_A, x=DW_X, H=H, L=L, Hx=Hx, G=G, scale_G=sG, scale_Hx=sHx)
    print(out, H.shape, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    folder = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wgrid")
    make_wgrid(folder)
    make_dwgrid(folder)
