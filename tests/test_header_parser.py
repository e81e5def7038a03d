"""The parser behind the binding (orb_slam2_ssd_semantic_amd/_header.py): every construct include/orbfe.h is written in, and an
error that names the declaration for everything else.  No GPU, no library."""
import ctypes as C

import numpy as np
import pytest

from orb_slam2_ssd_semantic_amd._header import Header, HeaderError

PRELUDE = """
#ifndef X_H
#define X_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef int32_t orbfe_status;
typedef struct orbfe_handle orbfe_handle; /* opaque */
#define ORBFE_N 3
typedef struct orbfe_rec { float a[ORBFE_N], b[3]; int32_t n; } orbfe_rec;
"""
EPILOGUE = """
#ifdef __cplusplus
}
#endif
#endif /* X_H */
"""


def parse(body, byref=()):
    return Header(PRELUDE + body + EPILOGUE, byref)


def test_prototypes():
    h = parse("""
int32_t orbfe_version(void);
const char *orbfe_name(orbfe_status s);
void orbfe_destroy(orbfe_handle *h);
void *orbfe_stream(orbfe_handle *h);
size_t orbfe_bytes(size_t n, double x, int64_t big, uint64_t id, const char *path, float f);
int64_t orbfe_count(const orbfe_handle *h);
double orbfe_ratio(void);
orbfe_status orbfe_create(const orbfe_rec *p, orbfe_handle **out);
orbfe_status orbfe_arrays(const uint8_t a[32], float ms[ORBFE_N], const uint8_t *const *rows, const uint32_t **off);
orbfe_status orbfe_long(orbfe_handle *h, const uint8_t *gray /* cap x 32 */, int32_t w,
                        int32_t ht,
                        orbfe_rec *recs,
                        int32_t *n_out);
""", byref=("orbfe_rec",))
    vp, i32 = C.c_void_p, C.c_int32
    rec = C.POINTER(h.structs["orbfe_rec"])
    assert h.prototypes == {
        "orbfe_version": (i32, []),
        "orbfe_name": (C.c_char_p, [i32]),
        "orbfe_destroy": (None, [vp]),
        "orbfe_stream": (vp, [vp]),
        "orbfe_bytes": (C.c_size_t, [C.c_size_t, C.c_double, C.c_int64, C.c_uint64, C.c_char_p, C.c_float]),
        "orbfe_count": (C.c_int64, [vp]),
        "orbfe_ratio": (C.c_double, []),
        "orbfe_create": (i32, [rec, vp]),
        "orbfe_arrays": (i32, [vp, vp, vp, vp]),
        "orbfe_long": (i32, [vp, vp, i32, i32, rec, vp]),
    }
    assert list(h.prototypes) == ["orbfe_version", "orbfe_name", "orbfe_destroy", "orbfe_stream", "orbfe_bytes", "orbfe_count",
                                  "orbfe_ratio", "orbfe_create", "orbfe_arrays", "orbfe_long"]
    assert h.opaque == {"orbfe_handle"}
    # without byref a pointer to the record is a plain address
    assert parse("orbfe_status orbfe_create(const orbfe_rec *p, orbfe_handle **out);").prototypes["orbfe_create"] == (i32, [vp, vp])


def test_structs():
    h = parse("""
typedef struct orbfe_outer {
    int32_t n;            /* then 4 bytes of padding: the double is 8-aligned */
    double d;
    orbfe_rec inner;      /* a nested record */
    const float *p, *q;   /* pointer members */
    uint8_t flag;
    int64_t big[2];
} orbfe_outer;
""")
    rec, outer = h.structs["orbfe_rec"], h.structs["orbfe_outer"]
    assert [(n, t) for n, t in rec._fields_] == [("a", C.c_float * 3), ("b", C.c_float * 3), ("n", C.c_int32)]
    assert [n for n, _ in outer._fields_] == ["n", "d", "inner", "p", "q", "flag", "big"]
    assert [getattr(outer, n).offset for n, _ in outer._fields_] == [0, 8, 16, 48, 56, 64, 72] and C.sizeof(outer) == 88
    assert outer.inner.size == C.sizeof(rec) == 28 and dict(outer._fields_)["p"] is C.c_void_p
    d = h.dtype("orbfe_outer")
    assert d.itemsize == 88 and [d.fields[n][1] for n in d.names] == [0, 8, 16, 48, 56, 64, 72]
    assert d["inner"] == h.dtype("orbfe_rec") == np.dtype([("a", "<f4", (3,)), ("b", "<f4", (3,)), ("n", "<i4")])
    assert d["p"] == np.dtype(np.uintp) and d["big"] == np.dtype(("<i8", (2,)))


def test_dtype_reshapes_without_resizing():
    h = parse("typedef struct orbfe_m { float T[16]; int32_t n; orbfe_rec r; } orbfe_m;")
    d = h.dtype("orbfe_m", T=(4, 4))
    assert d["T"].shape == (4, 4) and d.itemsize == h.dtype("orbfe_m").itemsize == 96 and d.fields["n"][1] == 64
    inner = np.dtype([("a", "<f4", (3,)), ("b", "<f4", (3, 1)), ("n", "<i4")])
    assert h.dtype("orbfe_m", r=inner)["r"]["b"].shape == (3, 1)
    with pytest.raises(ValueError, match="orbfe_m.T"):
        h.dtype("orbfe_m", T=(4, 3))
    with pytest.raises(ValueError, match="orbfe_m.r"):
        h.dtype("orbfe_m", r=np.dtype([("a", "<f4", (3,))]))
    with pytest.raises(KeyError):
        h.dtype("orbfe_m", nope=(1,))


def test_constants():
    h = parse("""
enum { ORBFE_A = 0, ORBFE_B = 1 };
enum {
    ORBFE_OPT_X = 1,   /* a comment, with a comma */
    ORBFE_OPT_Y = 2,
    /* 3 .. 15: reserved */
    ORBFE_OPT_Z = 16,
    ORBFE_NEG = -7,
    ORBFE_NEXT,
    ORBFE_SAME = ORBFE_N
};
#define ORBFE_HEX 0x20   /* a comment
                          * over two lines */
#define ORBFE_TH 100
""")
    assert h.constants == dict(ORBFE_N=3, ORBFE_A=0, ORBFE_B=1, ORBFE_OPT_X=1, ORBFE_OPT_Y=2, ORBFE_OPT_Z=16, ORBFE_NEG=-7, ORBFE_NEXT=-6,
                               ORBFE_SAME=3, ORBFE_HEX=32, ORBFE_TH=100)
    assert h.ORBFE_OPT_Z == 16
    with pytest.raises(AttributeError):
        h.ORBFE_MISSING


@pytest.mark.parametrize("body, named", [
    ("orbfe_status orbfe_f(unsigned n);", "orbfe_f.*unsigned"),                                  # an unknown type
    ("orbfe_status orbfe_f(orbfe_other *p);", "orbfe_f.*orbfe_other"),
    ("typedef struct orbfe_s { int32_t n; long m; } orbfe_s;", "orbfe_s.*long"),
    ("orbfe_status orbfe_f(int32_t n, void (*cb)(int32_t), void *user);", "orbfe_f"),             # a function-pointer parameter
    ("typedef struct orbfe_s { uint32_t lo : 4; uint32_t hi : 28; } orbfe_s;", "orbfe_s.*lo : 4"),   # a bit-field
    ("typedef union orbfe_u { int32_t i; float f; } orbfe_u;", "orbfe_u"),                        # a union
    ("typedef struct orbfe_s { int32_t kind; union { int32_t i; float f; } v; } orbfe_s;", "orbfe_s"),
    ("typedef struct orbfe_s { float a[ORBFE_UNKNOWN]; } orbfe_s;", "orbfe_s.*ORBFE_UNKNOWN"),     # an unknown array bound
    ("orbfe_status orbfe_f(float ms[ORBFE_UNKNOWN]);", "orbfe_f.*ORBFE_UNKNOWN"),
    ("static inline int32_t orbfe_f(int32_t x) { return x; }", "orbfe_f"),                        # not a plain prototype
    ("int32_t orbfe_f(int32_t x)\nint32_t orbfe_g(void);", "orbfe_f"),
    ("orbfe_status orbfe_f(orbfe_rec by_value);", "orbfe_f.*orbfe_rec"),
    ("typedef struct orbfe_s { int32_t n; } orbfe_t;", "orbfe_s"),
    ("typedef enum { ORBFE_P, ORBFE_Q } orbfe_e;", "orbfe_e"),
    ("enum { ORBFE_P = ORBFE_UNKNOWN };", "ORBFE_P.*ORBFE_UNKNOWN"),
    ("#define ORBFE_SCALE 1.5", "ORBFE_SCALE"),
    ("#define ORBFE_MAX(a, b) ((a) > (b) ? (a) : (b))", "ORBFE_MAX"),
    ("#if ORBFE_N > 2\nint32_t orbfe_f(void);\n#endif", "#if ORBFE_N"),
])
def test_unsupported_declarations_raise_by_name(body, named):
    with pytest.raises(HeaderError, match=named):
        parse(body)


def test_the_header_itself():
    """what the binding is built from: nothing of include/orbfe.h is left unparsed (anything else would have raised) and the
    package parses it once"""
    from orb_slam2_ssd_semantic_amd import _ffi, sim3
    h = _ffi.ABI
    assert len(h.prototypes) >= 201 and len(h.structs) >= 30 and len(h.constants) >= 122 and len(h.opaque) >= 13
    assert set(_ffi.BYREF) <= set(h.structs) and _ffi.SYMBOLS == tuple(h.prototypes)
    assert sim3.ABI is h
    assert _ffi.OPTIONS == dict(overlap=1, rows=2, rows_fast=3, rows_blur=4, blur_pieces=5, blur_updown=6, pyr_rows=7, qt_threads_0=8,
                                qt_threads_1=9, qt_threads_2=10, debug=11, blur_rounding=16, reuse_identical_input=17)
    assert h.prototypes["orbfe_get_stage_ms"] == (C.c_int32, [C.c_void_p, C.c_void_p])
    assert h.prototypes["orbfe_track_scratch_bytes"] == (C.c_int64, [C.c_int32, C.c_int32, C.c_int64])
    assert h.prototypes["orbfe_image_bounds"][1][0] is C.POINTER(_ffi.OrbfeCamera)
