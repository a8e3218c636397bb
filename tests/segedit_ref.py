"""NumPy / SciPy restatement of the segment edits (vx_segment_edit, DESIGN.md section 2 "Segment edits"), each op twice: with
scipy.ndimage, and independently with shifted copies in NumPy (segment_ref._dilate, erode by duality, fill by labelling the
background and dropping the components that touch a face).  Masks are bool arrays indexed [z, y, x].

The border rules are the contract's: a dilation reads voxels outside the volume as not set, an erosion reads them as set
(scipy's border_value=1, not its default), and open / close compose the two halves, each with its own rule."""
import numpy as np
from scipy import ndimage

from tests import segment_ref as SG

OPS = ("dilate", "erode", "open", "close", "fill_holes")


def structure(conn):
    return ndimage.generate_binary_structure(3, 1 if conn == 6 else 3)


# ---- scipy.ndimage ------------------------------------------------------------------------------------------------------
def sp_dilate(m, conn, n, band=None):
    if band is None:
        return ndimage.binary_dilation(m, structure(conn), iterations=n)
    # scipy's mask= keeps the input where mask is False and takes the dilation where it is True: with M not inside P the
    # contract's M | (D(M) & P) per step is the same thing, since D(M) holds M
    return ndimage.binary_dilation(m, structure(conn), iterations=n, mask=band)


def sp_erode(m, conn, n):
    return ndimage.binary_erosion(m, structure(conn), iterations=n, border_value=1)


def sp_open(m, conn, n):
    return sp_dilate(sp_erode(m, conn, n), conn, n)


def sp_close(m, conn, n):
    return sp_erode(sp_dilate(m, conn, n), conn, n)


def sp_fill(m, conn):
    return ndimage.binary_fill_holes(m, structure=structure(conn))


def scipy_edit(m, op, conn, n=1, band=None):
    m = np.asarray(m, dtype=bool)
    if op == "dilate":
        return sp_dilate(m, conn, n, band)
    if op == "erode":
        return sp_erode(m, conn, n)
    if op == "open":
        return sp_open(m, conn, n)
    if op == "close":
        return sp_close(m, conn, n)
    if op == "fill_holes":
        return sp_fill(m, conn)
    raise ValueError(op)


# ---- shifted copies -----------------------------------------------------------------------------------------------------
def np_dilate(m, conn, n, band=None):
    for _ in range(n):
        m = SG._dilate(m, conn) if band is None else m | (SG._dilate(m, conn) & band)
    return m


def np_erode(m, conn, n):
    """by duality: the complement inside the volume, dilated with the outside not set"""
    return ~np_dilate(~m, conn, n)


def np_fill(m, conn):
    """label the background, drop the components with a voxel on any of the six faces, add the rest"""
    bg = ~m
    lab, k = ndimage.label(bg, structure=structure(conn))
    faces = np.zeros_like(m)
    faces[0], faces[-1], faces[:, 0], faces[:, -1], faces[:, :, 0], faces[:, :, -1] = (True,) * 6
    open_labels = np.unique(lab[faces & bg])
    keep = np.ones(k + 1, dtype=bool)
    keep[0] = False
    keep[open_labels] = False
    return m | keep[lab]


def numpy_edit(m, op, conn, n=1, band=None):
    m = np.asarray(m, dtype=bool)
    if op == "dilate":
        return np_dilate(m, conn, n, band)
    if op == "erode":
        return np_erode(m, conn, n)
    if op == "open":
        return np_dilate(np_erode(m, conn, n), conn, n)
    if op == "close":
        return np_erode(np_dilate(m, conn, n), conn, n)
    if op == "fill_holes":
        return np_fill(m, conn)
    raise ValueError(op)


# the restatement the device is held to
edit = scipy_edit


# ---- shapes for the tests -----------------------------------------------------------------------------------------------
def blobs(shape, seed=0, sigma=2.5, q=0.6):
    """a blobby mask that touches the faces: smoothed noise above its q quantile"""
    rng = np.random.default_rng(seed)
    f = ndimage.gaussian_filter(rng.standard_normal(shape), sigma, mode="wrap")
    return f > np.quantile(f, q)


def shell(shape, lo, hi):
    """a hollow box: the voxels of [lo, hi] (inclusive, (x, y, z)) on its surface, one voxel thick"""
    m = np.zeros(shape, dtype=bool)
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    m[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] = True
    m[z0 + 1:z1, y0 + 1:y1, x0 + 1:x1] = False
    return m
