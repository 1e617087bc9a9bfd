"""Copies of a pyramid between contexts on the device (hsm_copy_map, hsm_copy_map_boxes, hsm_group_sync_maps): what can be
checked without a GPU.

* every new symbol is declared in capi.h, bound in capi.SIGNATURES with as many arguments, and exported by the built library; the
  header stays C99 and says what the boxes form assumes and which route has not been run;
* a NULL context or group is HSM_ERR_INVALID from each new entry, with the documented text (no device needed);
* the new unit is part of the build.
"""
import ctypes as C

from support import check_symbols, compile_c99, header_text

NEW_SYMBOLS = ("hsm_copy_map", "hsm_copy_map_boxes", "hsm_group_sync_maps")
HSM_ERR_INVALID = -1


def test_new_symbols_declared_bound_and_exported():
    from hector_slam_amd import build, capi
    check_symbols(NEW_SYMBOLS)
    head = header_text()
    assert "equalled `src` outside the boxes" in head and "HSM_COPY_STAGE=1" in head
    assert "the cross-device copy itself has not been run" in head and "address order" in head
    assert callable(capi.MapRepMultiMap.copy_map_from) and callable(capi.MapRepGroup.sync_maps)
    unit = build.UNITS["map_copy.hip"]
    assert any(d.endswith("map_copy_kernels.h") for d in unit) and any(d.endswith("map_copy_box.h") for d in unit)


def test_header_with_the_new_entries_is_plain_c99(tmp_path):
    compile_c99(tmp_path,
                "int main(void) { hsm_ctx* a = 0; hsm_ctx* b = 0; hsm_group* g = 0; int boxes[4] = {0, 0, -1, -1};\n"
                "  int rc = hsm_copy_map(a, b);\n"
                "  rc += hsm_copy_map_boxes(a, b, boxes);\n"
                "  rc += hsm_group_sync_maps(g, 0, boxes);\n"
                "  return rc; }\n")


def test_null_context_is_invalid_for_every_new_entry():
    from hector_slam_amd import capi
    lib = capi.load_library()
    boxes = (C.c_int * 32)()
    assert lib.hsm_copy_map(None, None) == HSM_ERR_INVALID
    assert b"null context" in lib.hsm_last_error()
    assert lib.hsm_copy_map_boxes(None, None, C.addressof(boxes)) == HSM_ERR_INVALID
    assert b"null context" in lib.hsm_last_error()
    assert lib.hsm_copy_map_boxes(None, None, None) == HSM_ERR_INVALID
    assert lib.hsm_group_sync_maps(None, 0, C.addressof(boxes)) == HSM_ERR_INVALID
    assert b"null group" in lib.hsm_last_error()
    assert lib.hsm_group_sync_maps(None, 0, None) == HSM_ERR_INVALID
