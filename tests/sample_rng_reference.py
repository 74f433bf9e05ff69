"""numpy restatement of the counter-based sampler draws (include/mapdit.h, "Counter-based sampler draws"): the sample-index / tag layout
and the label formula, on data_reference's Philox4x32-10, uniforms and fp64 normals.  Imports nothing from the package."""
import numpy as np

import data_reference as R

TAG_SMPZ, TAG_SMPN, TAG_SMPY = 0x534D505A, 0x534D504E, 0x534D5059      # "SMPZ", "SMPN", "SMPY"
U64 = np.uint64


def z0(seed, s, per):
    """The initial latent of sample index s, fp64 [per]: element i = normal i & 3 of counter (i >> 2, s, 0, TAG_SMPZ)."""
    return R.normals(seed, s, 0, TAG_SMPZ, per)


def noise(seed, s, t, per):
    """The noise of the step sample index s takes at schedule index t, fp64 [per]: counter (i >> 2, s, t, TAG_SMPN)."""
    return R.normals(seed, s, t, TAG_SMPN, per)


def labels(seed, index, num_classes):
    """y[s] = (uint64(w0) * num_classes) >> 32 of counter (0, s, 0, TAG_SMPY), int64 [len(index)]."""
    w = R.philox(0, np.asarray(index, dtype=U64), 0, TAG_SMPY, *R.key(seed))
    return ((w[0] * U64(num_classes)) >> U64(32)).astype(np.int64)
