"""Model sets on the host side: the new C-ABI entries are exported, bound and reject a NULL ctx without a GPU."""
import ctypes as C

from cova_amd import _lib as L

NEW = ["covahip_blobnet_load_set", "covahip_blobnet_num_models", "covahip_blobnet_forward_m", "covahip_filter_forward_m",
       "covahip_filter_forward_frames_m", "covahip_filter_forward_frames_packed_m"]


def test_model_set_entries_are_bound():
    lib = L.lib()
    for name in NEW:
        assert name in L.PROTOTYPES, name
        assert getattr(lib, name) is not None


def test_model_set_entries_reject_null_ctx():
    lib = L.lib()
    n = C.c_int()
    blob = C.c_char_p(b"x" * 64)
    ptrs = (C.c_char_p * 1)(b"x" * 64)
    sizes = (C.c_size_t * 1)(64)
    ids = (C.c_uint8 * 4)(0, 1, 0, 1)
    assert lib.covahip_blobnet_load_set(None, 1, ptrs, sizes, 68, 120, 4, 4) == 1
    assert lib.covahip_blobnet_num_models(None, C.byref(n)) == 1
    assert lib.covahip_blobnet_forward_m(None, blob, ids, 4, None, None, L.MEM_HOST) == 1
    assert lib.covahip_filter_forward_m(None, blob, ids, 4, 1, None, None, 0, None, None, L.MEM_HOST) == 1
    assert lib.covahip_filter_forward_frames_m(None, blob, 7, None, ids, 4, 1, None, None, 0, None, None, L.MEM_HOST) == 1
    assert lib.covahip_filter_forward_frames_packed_m(None, blob, 7, None, ids, 4, 1, None, None, 0, None, None) == 1
