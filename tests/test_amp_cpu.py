"""CPU: the fp16 precision mode's host side -- mode names, the (split_products, split_operand) pairs of the C ABI, install()."""
import inspect

import pytest


def test_precision_modes_and_install_signature():
    import cwfa_amd
    from cwfa_amd import ops
    assert "fp16" in ops.PRECISIONS
    assert "precision" in inspect.signature(cwfa_amd.install).parameters
    with pytest.raises(ValueError):
        ops.set_precision("fp8")


def test_option_pairs():
    from cwfa_amd import _lib, ops
    L = _lib.lib()
    try:
        ops.set_precision("fp16")
        assert ops.single_product()
        assert L.cwfa_set_option(b"split_products", 6) == -1           # (6, fp16) is refused
        ops.set_precision("split_bf16")
        assert not ops.single_product()
        assert L.cwfa_set_option(b"split_operand", 1) == -1            # ... from either side
        assert L.cwfa_set_option(b"split_operand", 2) == -1
        for mode in ("fp32", "fp16", "bf16", "split_bf16", "fp32", "fp16", "fp32"):
            ops.set_precision(mode)
    finally:
        ops.set_precision("fp32")
