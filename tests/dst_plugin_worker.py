"""Child process of tests/test_gpu_dst.py: three `step` calls of the registry's
`projection_hip` solver on the fields of an .npz file, with whatever
CFD_HIP_POISSON the parent set (the plugin reads it once, when it creates its
context), the results saved next to it.

usage: dst_plugin_worker.py IN.npz OUT.npz
"""
import sys

import numpy as np

from cfd_amd import _abi as A
from cfd_amd import _native, api


def main(src, dst):
    d = np.load(src)
    nx, ny, nz = (int(v) for v in d["shape"])
    box = d["box"]
    g = api.Grid(nx, ny, nz, 0.0, float(box[0]), 0.0, float(box[1]), 0.0, float(box[2]))
    f = api.FlowField(nx, ny, nz)
    for k in ("u", "v", "w", "p"):
        getattr(f, k)[...] = d[k]
    f.rho[...] = 1.0
    f.T[...] = 300.0
    prm = api.validation_params(float(d["dt"]), float(d["nu"]))
    solver = api.Registry().create("projection_hip")
    assert solver.init(g, prm) == A.CFD_SUCCESS, _native.last_error()
    st = A.SolverStats()
    for _ in range(int(d["steps"])):
        s = solver.step(f, g, prm, st)
        assert s == A.CFD_SUCCESS, (s, _native.last_error())
    np.savez(dst, u=f.u, v=f.v, w=f.w, p=f.p)
    solver.close()
    print("DST_PLUGIN_OK")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
