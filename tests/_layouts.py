"""Factor matrices as a caller may hand them over: rows `k + pad` elements apart, the first element `off` elements past a 16-byte
boundary, and a value nobody may read in every element that is not a factor.  Pure NumPy: nothing here is imported from the product.

The C-ABI gives every factor entry a leading dimension and takes any pointer.  tests/test_factor_layouts_cpu.py checks this helper
and the pair list without a GPU; tests/test_hip_factor_layouts.py hands the layouts to the device entries (which pass the stride
and the base on to the kernels) and to the host entries in several batches and shards (which step through the caller's rows by
`lda` before they compact them)."""
import numpy as np

# (pad, off) in elements, per precision
LAYOUTS = {
    "D": {"f32": (0, 0), "f64": (0, 0)},      # dense and aligned: the control
    "R1": {"f32": (1, 0), "f64": (1, 0)},     # odd stride: only some rows are 16-byte aligned
    "RA": {"f32": (4, 0), "f64": (2, 0)},     # every row 16-byte aligned, but ld != k
    "O1": {"f32": (0, 1), "f64": (0, 1)},     # dense rows, base one element past the boundary
    "RO": {"f32": (3, 1), "f64": (3, 1)},     # stride and offset together
}
# (layout of A, layout of B): every layout on each side, "aligned with a stride" and "unaligned" meet in both directions; with
# k = 16, O1 is the only layout with an unaligned base at a stride that is a multiple of 16 bytes
PAIRS = (("R1", "R1"), ("RA", "RA"), ("O1", "O1"), ("RO", "D"), ("D", "RO"), ("RA", "R1"), ("R1", "RA"), ("O1", "RA"), ("RA", "O1"))
CONTROL = ("D", "D")
TAIL = 16                                      # poisoned elements behind the last row (behind its `pad` elements)
# what the gaps hold: NaN where the point is "a gap is never read"; the largest finite magnitudes where max |x| (k_absmax) is looked
# at -- finite, so the non-finite flag stays down, but k * max|A| * max|B| is then far beyond the bound that lets the sweep skip its
# NaN scan
NAN_POISON = {"f32": np.float32(np.nan), "f64": np.float64(np.nan)}
BIG_POISON = {"f32": np.float32(3e38), "f64": np.float64(1.7e308)}
PREC = {np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}


def place(X, pad, off, poison):
    """(V, raw, at): V is a view into `raw` with V.shape == X.shape and V == X, rows X.shape[1] + pad elements apart, V[0, 0] =
    raw[at] lying `off` elements past a 16-byte boundary; every element of `raw` outside V holds `poison` (the `off` elements in
    front, `pad` behind each row, TAIL behind the last).  `raw` itself starts at a 16-byte boundary, so a copy of it to any buffer that
    does (a device allocation) keeps the alignment of V, and `at` == off."""
    X = np.asarray(X)
    assert X.ndim == 2 and pad >= 0 and off >= 0
    m, k = X.shape
    ld = k + pad
    size = off + m * ld + TAIL
    store = np.empty(size + 16 // X.itemsize, X.dtype)
    a0 = (-store.ctypes.data % 16) // X.itemsize                     # first 16-byte aligned element (NumPy aligns to the item size at least)
    raw = store[a0:a0 + size]
    assert raw.ctypes.data % 16 == 0 and raw.flags.c_contiguous
    raw[...] = poison
    at = off
    V = raw[at:at + m * ld].reshape(m, ld)[:, :k]
    V[...] = X
    return V, raw, at


def place_as(X, name, poison):
    """place() by the layout's name, for the precision of X"""
    pad, off = LAYOUTS[name][PREC[np.dtype(X.dtype)]]
    return place(X, pad, off, poison)


def outside(V, raw, at):
    """the elements of `raw` that are not elements of V, as a flat copy"""
    m, k = V.shape
    ld = V.strides[0] // V.itemsize
    inside = np.zeros(raw.shape[0], bool)
    inside[(at + np.arange(m)[:, None] * ld + np.arange(k)[None, :]).ravel()] = True
    return raw[~inside]
