"""Host build of rbvfit_amd/csrc/voigt_w_device.h: the device functions behind the gradient's per-pixel derivatives compiled for
the CPU, one lane per wave, and held against tests/golden/wgrid/dwgrid.npz (40 digits).  No GPU needed; it is how the series
lengths and switches of dw_generic were chosen and where the CPU-side table of profiles/grad_notes.md comes from.

The two headers are copied into a temporary folder with the HIP include and the one inline-assembly FMA replaced, and compiled
by clang++ (ROCm's, or $CXX) with -ffp-contract=off -mfma behind a shim that defines away the HIP qualifiers:
__ballot(p) is the one lane's own predicate, the hardware reciprocal is 1/d, erfcx comes from long double.  So a wave is
always tier-uniform (what the `banded` order of tests/test_gpu_grad_tiers.py arranges on the GPU); `--mixed` evaluates the fast
domain as a wave with core pixels in it does (core below 8, dw_wing<NWING + 1> from there).  libm's exp / sin / cos stand in for
the device library's in the two generic branches, so the last digit can differ from a GPU run.

    python scripts/dw_host_check.py [--mixed] [--generic-from-w]

--generic-from-w: outside the fast domain form the derivatives from w_generic's H and L at every |z| (the rule before
dw_generic), for the `before` column."""
import argparse
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rbvfit_amd", "csrc")
SHIM = r"""
#include <cmath>
#include <cstdint>
#include <cstddef>
#include <algorithm>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __builtin_amdgcn_rcp(d) (1.0 / (d))
#define __ballot(p) ((p) ? 1ull : 0ull)
using std::min; using std::max;
static inline double erfcx(double y) { return (double)(expl((long double)y * y) * erfcl((long double)y)); }
#include "voigt_w_device.h"
using namespace vp;
extern "C" void dw_host(int how, int n, const double* x, const double* a, double* H, double* Hx, double* G) {
    for (int i = 0; i < n; ++i) {
        const int mode = dw_mode(a[i]);
        const double ea2 = ea2_small(a[i]);
        const int nodd = core_terms(a[i]);
        DW d;
        if (mode != 0) d = (how & 2) ? dw_from_w(x[i], a[i], w_generic(x[i], a[i])) : dw_line(x[i], a[i], ea2, mode, nodd);
        else if (how & 1) d = fabs(x[i]) < X_CORE ? dw_from_w(x[i], a[i], w_core_taylor(x[i], a[i], ea2, nodd)) : dw_wing<NWING + 1>(x[i], a[i]);
        else d = dw_line(x[i], a[i], ea2, mode, nodd);
        H[i] = d.H; Hx[i] = d.Hx; G[i] = d.G;
    }
}
"""
BANDS = [(0, 6), (6, 8), (8, 15), (15, 36), (36, 140), (140, 600), (600, 1e4), (1e4, np.inf)]


def build(folder):
    with open(os.path.join(CSRC, "voigt_device.h")) as f:
        text = f.read().replace("#include <hip/hip_runtime.h>", "")
    text, n = re.subn(r'asm\("v_fma_f64[^;]*;', "d = __builtin_fma(a, b, c_uniform);", text)
    assert n == 1
    with open(os.path.join(folder, "voigt_device.h"), "w") as f:
        f.write(text)
    for name in ("dawson_table.h", "voigt_w_device.h"):
        with open(os.path.join(CSRC, name)) as src, open(os.path.join(folder, name), "w") as dst:
            dst.write(src.read())
    with open(os.path.join(folder, "shim.cpp"), "w") as f:
        f.write(SHIM)
    hipcc = os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    cxx = os.environ.get("CXX") or os.path.join(os.path.dirname(os.path.dirname(hipcc)), "lib", "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        cxx = "clang++"
    lib = os.path.join(folder, "libdwhost.so")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-o", lib, "shim.cpp"], check=True, cwd=folder)
    return C.CDLL(lib)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mixed", action="store_true")
    ap.add_argument("--generic-from-w", action="store_true")
    args = ap.parse_args()
    z = np.load(os.path.join(ROOT, "tests", "golden", "wgrid", "dwgrid.npz"))
    a, x = z["a"], z["x"]
    A, X = (np.ascontiguousarray(v.ravel()) for v in np.meshgrid(a, x, indexing="ij"))
    out = [np.empty(A.size) for _ in range(3)]
    dp = C.POINTER(C.c_double)
    with tempfile.TemporaryDirectory() as folder:
        lib = build(folder)
        lib.dw_host(int(args.mixed) + 2 * int(args.generic_from_w), A.size, *(v.ctypes.data_as(dp) for v in [X, A] + out))
    floor = 1e-17 * ((a[:, None] == 0) & (np.abs(x)[None, :] >= 8.0))
    ratio = []
    for got, name, scale in zip(out, ("H", "Hx", "G"), (np.abs(z["H"]), z["scale_Hx"], z["scale_G"])):
        err = np.abs(got.reshape(a.size, x.size) - z[name])
        ratio.append(np.where(err <= floor, 0.0, err / np.maximum(scale, 1e-300)))
    print("worst error / scale (bounds: 1e-12 for H, 1e-10 for Hx and G)")
    for label, sel in (("0 <= a <= 0.1", a <= 0.1), ("0.1 < a < 7", (a > 0.1) & (a < 7)), ("a >= 7", a >= 7)):
        for lo, hi in BANDS:
            m = sel[:, None] & ((np.abs(x) >= lo) & (np.abs(x) < hi))[None, :]
            print("  %-14s |x| in [%g, %g): H %.2e  Hx %.2e  G %.2e" % (label, lo, hi, ratio[0][m].max(), ratio[1][m].max(), ratio[2][m].max()))


if __name__ == "__main__":
    main()
