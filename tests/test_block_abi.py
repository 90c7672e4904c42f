"""The block products (krcn_matvec_block / krcn_rmatvec_block / krcn_hvp_block)
load and validate their arguments on the host, before any HIP call: no GPU needed."""
BLOCK = ("krcn_matvec_block", "krcn_rmatvec_block", "krcn_hvp_block")


def test_symbols_and_signatures():
    from krcn import _lib
    lib = _lib.load()
    for name in BLOCK:
        assert hasattr(lib, name), f"libkrcn.so does not export {name}"
        assert name in _lib.SIGNATURES
    assert _lib.KRCN_BLOCK_MAX == 16
    assert _lib.KRCN_BLOCK_LONG_ROW == 512


def test_constants_match_the_header():
    import os
    import re

    from conftest import REPO
    from krcn import _lib
    text = open(os.path.join(REPO, "include", "krcn.h")).read()
    m = re.search(r"KRCN_BLOCK_MAX = (\d+), KRCN_BLOCK_LONG_ROW = (\d+)", text)
    assert m, "include/krcn.h does not define the block constants"
    assert (int(m.group(1)), int(m.group(2))) == (_lib.KRCN_BLOCK_MAX, _lib.KRCN_BLOCK_LONG_ROW)


def test_null_handle_is_invalid_before_any_hip_call():
    from krcn import _lib
    lib = _lib.load()
    assert lib.krcn_matvec_block(None, 2, None, None, None) == _lib.KRCN_ERR_INVALID
    assert b"null handle" in lib.krcn_last_error_string()
    assert lib.krcn_rmatvec_block(None, 2, None, None, None) == _lib.KRCN_ERR_INVALID
    assert b"null handle" in lib.krcn_last_error_string()
    assert lib.krcn_hvp_block(None, 2, None, 1, None, None, None, None) == _lib.KRCN_ERR_INVALID
    assert b"null handle" in lib.krcn_last_error_string()
