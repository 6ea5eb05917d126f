"""CPU: which head sizes the flash kernels of csrc/attn_hd.hip take in bf16 mode (every multiple of 4 from 4 to 128), at the
functional, the ops and the library level; and the entry points are still the two of ABI version 11 -- declared in the header, bound
in _lib.SIGNATURES with the header's argument counts, exported by the library."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gaot_attn_hd_fwd", "gaot_attn_hd_bwd")
ELIGIBLE = (4, 16, 20, 48, 68, 96, 100, 128)
NOT_ELIGIBLE = (2, 6, 50, 132, 256)


def test_hd_flash_predicate():
    from gaot_3d_amd import functional as GF
    for d in ELIGIBLE:
        assert GF.hd_flash_eligible(d), d
    for d in NOT_ELIGIBLE + (0, -4):
        assert not GF.hd_flash_eligible(d), d
    assert GF.hd_flash_eligible(32)            # at the ops level; inside the model head size 32 keeps AttentionFn
    assert GF.HD_FLASH_HEAD_DIMS == tuple(range(4, 129, 4))
    assert all(GF.hd_flash_eligible(d) == (d in GF.HD_FLASH_HEAD_DIMS) for d in range(-8, 300))


def test_ops_apply_the_same_rule():
    from gaot_3d_amd import functional as GF, ops
    assert all(ops.attn_hd_head_dim_ok(d) == GF.hd_flash_eligible(d) for d in range(-8, 300))
    assert "multiple of 4" in ops.HD_HEAD_DIM_RULE and "128" in ops.HD_HEAD_DIM_RULE


@pytest.mark.parametrize("d", NOT_ELIGIBLE)
def test_library_refuses_other_head_sizes_by_the_rule(d):
    """the C entry points check head_dim first and return the argument error, naming the rule, without touching a pointer"""
    from gaot_3d_amd import _lib
    lib = _lib.load()
    err_arg = 1       # GAOT_ERR_ARG (include/gaot3d_hip.h)
    rc = lib.gaot_attn_hd_fwd(None, None, None, None, None, 0, 0, 0, 0, 1, 4, 2, 2, d, 1.0, 0.0, None, 0, 0, None)
    assert rc == err_arg and b"gaot_attn_hd_fwd: head_dim must be a multiple of 4 with 4 <= head_dim <= 128" in lib.gaot_last_error()
    rc = lib.gaot_attn_hd_bwd(*([None] * 10), *([0] * 8), 1, 4, 2, 2, d, 1.0, 0.0, None, 0, 0, 7, None)
    assert rc == err_arg and b"gaot_attn_hd_bwd: head_dim must be a multiple of 4 with 4 <= head_dim <= 128" in lib.gaot_last_error()


def test_library_accepts_the_new_range_up_to_the_next_check():
    """an eligible head size passes the head_dim check: the call is then refused for its null pointers, not for its head size"""
    from gaot_3d_amd import _lib
    lib = _lib.load()
    for d in ELIGIBLE + (32, 64):
        rc = lib.gaot_attn_hd_fwd(None, None, None, None, None, 0, 0, 0, 0, 1, 4, 2, 2, d, 1.0, 0.0, None, 0, 0, None)
        assert rc != 0 and b"null pointer" in lib.gaot_last_error(), (d, lib.gaot_last_error())


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gaot3d_hip.h")).read(), flags=re.S)


def test_attn_hd_symbols_declared_bound_and_exported():
    from gaot_3d_amd import _lib
    src = _header()
    lib = _lib.load()
    for name in NAMES:
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src)
        assert m, f"{name} is not declared in include/gaot3d_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), f"{name}: header and SIGNATURES disagree on the arguments"
        assert hasattr(lib, name), f"{name} is not exported by libgaot3d_hip.so"
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("gaot_attn_hd")) == sorted(NAMES)     # no new symbol
    assert lib.gaot_abi_version() == 11
