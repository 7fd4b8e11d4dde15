"""Regenerates tests/golden/wgrid/wgrid.npz (a folder of its own: conftest.golden_cases() takes every .npz directly under
tests/golden for an lnprob fixture): w(x + i a) = exp(-z^2) erfc(-i z) at 40 digits (mpmath 1.3.0), stored as
float64 H = Re w and L = Im w.  The (a, x) values sit on and beside every tier boundary of the device evaluation
(rbvfit_amd/csrc/voigt_w_device.h).  Needs mpmath; the tests only read the .npz."""
import os

import mpmath
import numpy as np

mpmath.mp.dps = 40

A = np.array([0.0, 1e-6, 1e-3, 0.05, 0.1, np.nextafter(0.1, 1.0), 1.0, 7.0, 20.0])
XPOS = np.array([0.0, 1e-8, 1e-3, 0.1, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 2.5, 3.0, 3.7, 4.0, 4.99, 5.0, 5.5, 5.9, np.nextafter(6.0, 0.0), 6.0,
                 6.1, 7.0, 7.2, 7.49, 7.9, np.nextafter(8.0, 0.0), 8.0, np.nextafter(8.0, 9.0), 8.5, 9.0, 12.0, 14.0, 14.99, 15.0, 20.0,
                 30.0, 35.9, 36.0, 50.0, 100.0, 139.0, 140.0, 500.0, 599.0, 600.0, 3000.0, 9999.0, 1e4])
X = np.concatenate([-XPOS[:0:-1], XPOS])


def w(x, a):
    z = mpmath.mpc(mpmath.mpf(float(x)), mpmath.mpf(float(a)))
    return mpmath.exp(-z * z) * mpmath.erfc(-1j * z)


if __name__ == "__main__":
    H = np.empty((A.size, X.size))
    L = np.empty((A.size, X.size))
    for i, a in enumerate(A):
        for j, x in enumerate(X):
            v = w(x, a)
            H[i, j] = float(v.real)
            L[i, j] = float(v.imag)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wgrid", "wgrid.npz")
    np.savez_compressed(out, a=A, x=X, H=H, L=L)
    print(out, H.shape, os.path.getsize(out), "bytes")
