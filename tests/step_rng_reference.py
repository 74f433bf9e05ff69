"""numpy restatement of the counter-based step draws (include/mapdit.h, "Counter-based step draws"): the slot / tag layout and the integer
formulas, on data_reference's Philox4x32-10, uniforms and fp64 normals.  Imports nothing from the package."""
import math

import numpy as np

import data_reference as R

TAG_EPS, TAG_SYNX, TAG_STEP = 0x53455053, 0x53594E58, 0x53544550       # "SEPS", "SYNX", "STEP" - not TAG_PERM, not TAG_NOISE
U64 = np.uint64


def drop_threshold(p):
    """ceil(float32(p) * 2^24): exact in fp64 (an fp32 value times a power of two)."""
    return math.ceil(float(np.float32(p)) * 2.0 ** 24)


def plane(seed, step, slot, tag, per):
    """eps / x_syn of one slot, fp64 [per]: element i = normal i & 3 of counter (i >> 2, slot, step, tag)."""
    return R.normals(seed, slot, step, tag, per)


def planes(seed, step, first_slot, count, tag, per):
    return np.stack([plane(seed, step, first_slot + j, tag, per) for j in range(count)])


def scalars(seed, step, first_slot, count, T=1000, num_classes=10, drop_prob=0.1):
    """{t, drop, u, y_syn, z} of slots [first_slot, first_slot + count); z in fp64 from the same words."""
    slots = np.arange(first_slot, first_slot + count, dtype=U64)
    a = R.philox(0, slots, step, TAG_STEP, *R.key(seed))
    b = R.philox(1, slots, step, TAG_STEP, *R.key(seed))
    ur, ua = R.uniforms(b[2]), R.uniforms(b[3])
    return {"t": ((a[0] * U64(T)) >> U64(32)).astype(np.int64),
            "drop": ((a[1] >> U64(8)) < U64(drop_threshold(drop_prob))).astype(np.int64),
            "u": ((a[2] << U64(21)) | (a[3] >> U64(11))).astype(np.float64) * 2.0 ** -53,
            "y_syn": ((b[0] * U64(num_classes)) >> U64(32)).astype(np.int64),
            "z": np.sqrt(-2.0 * np.log(ur)) * np.cos(2.0 * np.pi * ua)}
