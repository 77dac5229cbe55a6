"""tools/isa_diff.py, the kernel-by-kernel comparison of two builds (CPU only): identity of the
built library against itself, a difference for one edited instruction line, and none for
padding appended after a kernel's last s_endpgm.  Works on the parsed dictionaries; builds no
second library."""
import copy
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_check  # noqa: E402
import isa_diff  # noqa: E402

pytestmark = pytest.mark.skipif(
    not os.path.exists(isa_check.LIB) or not os.path.exists(os.path.join(isa_check.LLVM, "llvm-objdump")),
    reason="needs the built library and the ROCm LLVM tools")


@pytest.fixture(scope="module")
def lib():
    return isa_diff.load(isa_check.LIB)


def _kernel(fns, meta):
    return next(k for k in sorted(meta) if isa_check.mtd_instance(k) == (128, 5, 1, 1) and len(fns[k]) > 100)


def test_library_equals_itself(lib):
    fns, meta = lib
    assert len(meta) > 100 and set(meta) <= set(fns)
    assert all(set(m) == set(isa_diff.META) for m in meta.values())
    assert isa_diff.diff(fns, fns, meta, meta) == []
    assert isa_diff.trim(fns[_kernel(fns, meta)])[-1].startswith("s_endpgm")


def test_edited_instruction_is_reported(lib):
    fns, meta = lib
    k = _kernel(fns, meta)
    new = copy.copy(fns)
    new[k] = list(fns[k])
    new[k][50] = "s_nop 7"
    probs = isa_diff.diff(fns, new, meta, meta)
    assert len(probs) == 1 and k in probs[0] and probs[0].startswith("instructions differ")
    # a changed descriptor and a missing kernel are differences too
    m2 = copy.deepcopy(meta)
    m2[k][".vgpr_count"] = str(int(meta[k][".vgpr_count"]) + 1)
    assert any(p.startswith("descriptor differs") and k in p for p in isa_diff.diff(fns, fns, meta, m2))
    del m2[k]
    assert any(p.startswith("only in OLD") and k in p for p in isa_diff.diff(fns, fns, meta, m2))


def test_trailing_padding_is_ignored(lib):
    fns, meta = lib
    k = _kernel(fns, meta)
    new = copy.copy(fns)
    new[k] = list(fns[k]) + ["s_nop 0"] * 40 + ["..."]
    assert isa_diff.diff(fns, new, meta, meta) == []
    new[k] = isa_diff.trim(fns[k])
    assert isa_diff.diff(fns, new, meta, meta) == []
