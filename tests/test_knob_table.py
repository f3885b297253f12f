"""The switch table of INTEGRATION.md section 2 lists exactly the MVAE_* environment switches the code reads:
every name inside an os.environ / getenv( read of the package's Python or csrc/, and nothing else."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "medvae_disentangled_multimodal_amd")
NAME = r"(MVAE_[A-Z0-9_]+)"
READ = re.compile(r"(?:os\.environ(?:\.get\(|\[)|getenv\()\s*\"" + NAME + "\"")
NOT_A_SWITCH = re.compile(r"MVAE_(CONV_|E|OK$)")  # constants of include/medvae_hip.h


def _text(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _read_in_code():
    files = glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True) + glob.glob(os.path.join(PKG, "csrc", "*"))
    assert len(files) > 30
    names = {m for f in files for m in READ.findall(_text(f))}
    return {n for n in names if not NOT_A_SWITCH.match(n)}


def _in_table():
    sec = _text(os.path.join(ROOT, "INTEGRATION.md")).split("\n## 2.", 1)[1].split("\n## 3.", 1)[0]
    rows = [r for r in sec.splitlines() if r.startswith("|")][2:]  # (after the header and its rule)
    assert len(rows) > 30
    return {n for r in rows for n in re.findall(NAME, r.split("|")[1])}


def test_switch_table_matches_the_code():
    code, table = _read_in_code(), _in_table()
    assert len(code) > 40
    assert sorted(code - table) == [], "read by the code, not in INTEGRATION.md section 2"
    assert sorted(table - code) == [], "in INTEGRATION.md section 2, read nowhere"
