"""(diagnostic) cycle stamps of the refinement path of the projection kernel, block 0 of a launch, from a -DNNSDP_STAMPS build of the
library that is never shipped:
    hipcc -O3 --offload-arch=gfx950 -fPIC -shared -std=c++17 -pthread -DNNSDP_STAMPS nn-sdp_amd/csrc/api.hip -o nn-sdp_amd/nnsdp_amd/libnnsdp_hip_stamps.so -lrocsolver -lrocblas -ldl
usage: python tools/refine_stamps.py [n=85] [blocks=19] [carry]     (carry: the per-block state travels from launch to launch as in a
solver, so launches 1 and 2 of every case run on the credit of launch 0 - without the Gram product)
With NNSDP_SPLIT_WARM=<H> in the environment the launches run H helper workgroups per block, and the build also prints wave 0 of
helpers 1 and nt - 1 of block 0 beside the leader's lines: loads issued / landed and stored / barrier / symmetrise / barrier, then T,
the B chains, the drained stores and the release (the helpers' printf delays their release: the leader's wait is longer than without)."""
import sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nn-sdp_amd")); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import numpy as np, nnsdp_amd as na
from nnsdp_amd import _lib
_lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libnnsdp_hip_stamps.so")
_lib._lib = None

n = int(sys.argv[1]) if len(sys.argv) > 1 else 85
nb = int(sys.argv[2]) if len(sys.argv) > 2 else 19
carry = len(sys.argv) > 3 and sys.argv[3] == "carry"
rng = np.random.default_rng(0)
def sym(n):
    spec = np.concatenate([np.linspace(0.2, 2.0, n - n // 3), -np.linspace(0.1, 1.5, n // 3)])
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (Q * spec) @ Q.T, Q
def perturb(A, eta):
    D = rng.standard_normal(A.shape); D = 0.5 * (D + D.T)
    return A + eta * np.linalg.norm(A) / np.linalg.norm(D) * D

base = [sym(n) for _ in range(nb)]
for name, eta, tol, refine in (("one refinement step", 1e-6, 3e-7, True), ("converged as given", 0.0, 1e-7, True), ("sweeps only (1 sweep)", 1e-6, 3e-7, False)):
    mats = [perturb(A, eta) if eta > 0 else A for A, _ in base]
    state = np.zeros(4 * nb, dtype=np.int32) if carry else None
    for rep in range(3):
        print(f"--- {name}, launch {rep}", flush=True)
        W, V, oc, ms = na.project_psd_warm(mats, [Q for _, Q in base], tol, refine=refine, state=state)
        print(f"    outcome {oc} kernel {1e3 * ms:.1f} us (2.4 GHz: {2.4e3 * 1e3 * ms:.0f} cycles)", flush=True)
