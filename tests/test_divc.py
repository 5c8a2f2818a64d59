"""The correctly rounded constant-divisor division of the relaxation sweeps
(device_util.hpp `divc`): tools/divc_check.c restates it on the host and compares
it bit for bit with `/` over random quotients for the grid spacings the tests
and BASELINE configs use (the full 9.6e8-quotient run is recorded in
DESIGN.md; here 1e6 per divisor)."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_divc_matches_division(tmp_path):
    exe = tmp_path / "divc_check"
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-o", str(exe),
                    str(ROOT / "tools" / "divc_check.c"), "-lm"], check=True)
    out = subprocess.run([str(exe), "1000000"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout
    assert "48000000 quotients, 0 mismatches" in out.stdout
