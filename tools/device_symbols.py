#!/usr/bin/env python3
"""One sorted line per device function of a built library: name, size and
sha256 of the symbol's bytes in .text, over every gfx950 code object.

A host-only change may reorder the kernels inside a code object (the order
follows the host code's first reference to each instantiation), which moves
cfd_amd._sha.device_code_sha although no kernel changed. Two libraries with
the same output here hold the same device functions:

    python3 tools/device_symbols.py old/libcfd_hip.so > a
    python3 tools/device_symbols.py cfd_amd/lib/libcfd_hip.so > b && cmp a b

--order lists the symbols by code object and address instead.
"""
import hashlib
import os
import subprocess
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "cfd_amd"))
import _sha  # noqa: E402

READELF = os.environ.get("LLVM_READELF", "/opt/rocm/llvm/bin/llvm-readelf")


def symbols(co: bytes):
    """(address, name, size, sha256 of the bytes) of every FUNC symbol in .text."""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(co)
        f.flush()
        out = subprocess.run([READELF, "-sW", "-S", f.name], check=True, capture_output=True,
                             text=True).stdout
    text = None  # (section index, address, file offset)
    for line in out.splitlines():
        w = line.replace("[", " ").replace("]", " ").split()
        if len(w) > 4 and w[1] == ".text" and w[2] == "PROGBITS":
            text = (w[0], int(w[3], 16), int(w[4], 16))
        elif len(w) == 8 and w[3] == "FUNC" and text and w[6] == text[0]:
            addr, size = int(w[1], 16), int(w[2])
            off = addr - text[1] + text[2]
            yield addr, w[7], size, hashlib.sha256(co[off:off + size]).hexdigest()


def main(argv):
    order = "--order" in argv
    lib = [a for a in argv if not a.startswith("--")][0]
    data = Path(lib).read_bytes()
    rows = []
    for off, size in _sha._elf_sections(data).get(".hip_fatbin", []):
        for n, (triple, co) in enumerate(_sha._offload_bundles(data[off:off + size])):
            if "gfx950" in triple:
                rows += [(off, n) + s for s in symbols(co)]
    if order:
        rows.sort()
    else:
        rows.sort(key=lambda r: r[3:])
    for r in rows:
        print(r[3], r[4], r[5])
    print(f"{len(rows)} function symbols", file=sys.stderr)


if __name__ == "__main__":
    main(sys.argv[1:])
