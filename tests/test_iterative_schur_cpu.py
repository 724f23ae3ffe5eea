"""BA_ITERSCHUR without a GPU: the library exports its entry points, the header names the kind, and the host structure the dense
symbols use is unchanged by the structure builder's new flag (ba_shard_plan returns the numbers it returned before the flag)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ba_mi355x.h")
NEW_SYMBOLS = ("ba_solver_set_pcg", "ba_solver_pcg_stats", "ba_solver_device_bytes")


@pytest.mark.skipif(shutil.which("nm") is None, reason="nm not available")
def test_library_exports_the_pcg_entry_points(ba):
    out = subprocess.run(["nm", "-D", "--defined-only", ba.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    missing = [s for s in NEW_SYMBOLS if s not in defined]
    assert not missing, missing
    assert all(s in ba.EXPORTS for s in NEW_SYMBOLS)
    assert ba.ITERSCHUR == 5 and ba.KIND_NAMES[ba.ITERSCHUR] == "ITERSCHUR"


def test_header_defines_iterschur_as_5():
    text = open(HEADER).read()
    m = re.search(r"typedef enum \{([^}]*)\} ba_solver_kind;", text)
    assert m, "ba_solver_kind not found"
    kinds = dict((k.strip(), int(v)) for k, v in re.findall(r"(\w+)\s*=\s*(\d+)", m.group(1)))
    assert kinds == {"BA_QRKIT": 0, "BA_QRCHOL": 1, "BA_CHOLESKY": 2, "BA_MOREQR": 3, "BA_QRSPQR": 4, "BA_ITERSCHUR": 5}, kinds
    for decl in ("int ba_solver_set_pcg(ba_solver *s, int max_iter, double rel_tol);",
                 "int ba_solver_pcg_stats(ba_solver *s, ba_pcg_stats *out, int reset);",
                 "int ba_solver_device_bytes(const ba_solver *s, size_t *bytes);"):
        assert decl in text, decl
    assert re.search(r"#define BA_PCG_MAX_ITER_DEFAULT \d+", text) and re.search(r"#define BA_PCG_REL_TOL_DEFAULT [0-9.e-]+", text)


# ba_shard_plan of the library before BA_ITERSCHUR existed: {p0, p1, o0, o1, entries, chunks, camera pairs, was_sorted}
PLAN_BEFORE = {
    ("p21", 0, 1): (0, 11315, 0, 36455, 96309, 1610, 231, 1),
    ("p21", 1, 3): (3220, 6545, 12156, 24304, 34113, 655, 231, 1),
    ("p39", 0, 1): (0, 18060, 0, 63551, 197397, 3426, 780, 1),
    ("p39", 1, 3): (4576, 9794, 21189, 42368, 71754, 1480, 780, 1),
}


@pytest.mark.parametrize("key", sorted(PLAN_BEFORE), ids=["%s-%d-of-%d" % k for k in sorted(PLAN_BEFORE)])
def test_shard_plan_unchanged(prob21, prob39, key):
    name, rank, world = key
    p = prob21 if name == "p21" else prob39
    got = p.shard_plan(rank, world)
    keys = ("p0", "p1", "o0", "o1", "entries", "chunks", "pairs", "was_sorted")
    assert tuple(got[k] for k in keys) == PLAN_BEFORE[key], got
