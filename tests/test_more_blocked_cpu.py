"""Host-side checks of the MORE route for blocked-path dimensions (no GPU needed)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("d", [1, 20, 63, 129, 300])
def test_more_blocked_refuses_dimensions_outside_its_range_without_a_device(d):
    """The range check comes first: no context, no array is touched."""
    from gmmvi_amd import hip_ops
    with pytest.raises(ValueError, match="64 <= D <= 128"):
        hip_ops.more_blocked(None, None, None, None, None, None, None, None, None, d)


def test_header_declares_the_blocked_more_entry_point():
    from gmmvi_amd import _lib
    header = open(os.path.join(ROOT, "include", "gmmvi_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+gmmvi_more_blocked\s*\(", code)
    assert re.search(r"#define\s+GMMVI_MORE_BLOCKED_MAX_DIM\s+128\b", code)
    assert "gmmvi_more_blocked" in _lib.EXPORTED_SYMBOLS
    assert len(_lib._PROTOS["gmmvi_more_blocked"][1]) == len(_lib._PROTOS["gmmvi_more"][1])
    assert (_lib.MORE_BLOCKED_MIN_DIM, _lib.MORE_BLOCKED_MAX_DIM) == (64, 128)
