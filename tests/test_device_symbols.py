"""Every device function of libcfd_hip.so is emitted by one translation unit:
no function name occurs in more than one gfx950 code object, and the kernels
bench.py keys on are there under the names the profiler prints. CPU only:
reads the built library with the functions of tools/device_symbols.py."""
import importlib.util
import os
import shutil
import subprocess
from pathlib import Path

import pytest

from cfd_amd import _sha
from cfd_amd._native import HIP_LIB

ROOT = Path(__file__).resolve().parent.parent
BENCH_KERNELS = ["k_pred3<false, 0>", "k_corr3<0>", "k_cg_setup<true, false, true, false>",
                 "k_ccf<false, false, false>", "k_cg_small"]


def _tool():
    spec = importlib.util.spec_from_file_location("device_symbols",
                                                  ROOT / "tools" / "device_symbols.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def code_objects():
    """The set of function names of each gfx950 code object of the library."""
    if not HIP_LIB.exists():
        pytest.skip("libcfd_hip.so not built")
    ds = _tool()
    if not os.access(ds.READELF, os.X_OK):
        pytest.skip("llvm-readelf not found")
    data = HIP_LIB.read_bytes()
    objs = []
    for off, size in _sha._elf_sections(data).get(".hip_fatbin", []):
        for triple, co in _sha._offload_bundles(data[off:off + size]):
            if "gfx950" in triple:
                objs.append({name for _, name, _, _ in ds.symbols(co)})
    return objs, ds.READELF


def test_each_device_function_in_one_code_object(code_objects):
    objs, _ = code_objects
    assert len(objs) > 1 and all(objs)
    owner = {}
    twice = []
    for n, names in enumerate(objs):
        for name in names:
            if name in owner:
                twice.append((name, owner[name], n))
            owner[name] = n
    assert not twice, f"device functions emitted by more than one unit: {sorted(twice)[:8]}"


def test_bench_kernels_present_under_their_printed_names(code_objects):
    objs, readelf = code_objects
    cxxfilt = shutil.which("llvm-cxxfilt", path=str(Path(readelf).parent)) or \
        shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not cxxfilt:
        pytest.skip("no C++ demangler (llvm-cxxfilt, c++filt) found")
    mangled = sorted(set().union(*objs))
    # -p: no parameter lists
    out = subprocess.run([cxxfilt, "-p"], input="\n".join(mangled), check=True,
                         capture_output=True, text=True).stdout.split("\n")
    # "void cfdhip::k_pred3<false, 0>" -> "k_pred3<false, 0>"
    printed = {d.split(" ", 1)[-1].replace("cfdhip::", "") if d.startswith("void ") else
               d.replace("cfdhip::", "") for d in out}
    for k in BENCH_KERNELS:
        assert k in printed, k
