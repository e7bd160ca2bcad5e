"""The manhattan and hamming metrics at the ABI and the binding (no GPU needed)."""
import ctypes as C

import weaviate_amd as W
from weaviate_amd import _lib


def test_metrics_in_binding_and_header():
    assert _lib.METRICS["manhattan"] == 3 and _lib.METRICS["hamming"] == 4
    header = open(_lib.HEADER).read()
    assert "WV_MANHATTAN = 3" in header and "WV_HAMMING = 4" in header


def test_mirror_and_unknown_metric_are_einval():
    out = C.c_void_p()
    assert W.lib().wv_mirror_create(3, None, None, C.byref(out)) == _lib.WV_EINVAL
    assert W.lib().wv_index_create(8, 5, None, 16, C.byref(out)) == _lib.WV_EINVAL
    assert not out.value
