"""Child process of tests/test_gpu_shell_transfers.py: the resident run of its
download case (tests/shell_cases.py, download_run: RB-SOR capped at 20
iterations, energy on) at one shape, with whatever CFD_HIP_SHELL_THREADS the
parent set (the library reads it once per process), the host arrays after
every step and after hip_proj_sync_host saved to an .npz file.

usage: shell_transfer_worker.py NXxNYxNZ OUT.npz
"""
import sys

import numpy as np

from cfd_amd import _abi as A
from tests import shell_cases as S


def main(shape, dst):
    shape = tuple(int(v) for v in shape.split("x"))
    res, synced = S.download_run(shape, True, True, poisson_method=A.HIP_POISSON_REDBLACK,
                                 poisson_max_iter=20, poisson_fail_fatal=0)
    out = {f"{n}_synced": a for n, a in synced.items()}
    for step, rec in enumerate(res):
        out[f"status{step}"] = np.array(rec["status"])
        out.update({f"{n}{step}": a for n, a in rec["host"].items()})
    np.savez(dst, **out)
    print("SHELL_TRANSFER_OK")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
