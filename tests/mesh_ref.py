"""NumPy restatement of the mesher (vx_mesh_extract, DESIGN.md section 2 "Meshes"): naive surface nets, every number an fp32 add,
subtract or divide in the stated order.  Written from the contract, not from the kernels.  Arrays are indexed [z, y, x]; cells,
vertices and boxes are (x, y, z).  A cell c has the corners c + {0, 1}^3 and c_a runs over [-1, extent_a - 1]: the padded arrays
below carry one phantom voxel (outside, f = 0) on every side, so cell c sits at padded index c + 1."""
import numpy as np

F32 = np.float32
BOX_END = 0xffffffff


def _padded(inside, f, box):
    Z, Y, X = inside.shape
    I = np.zeros((Z + 2, Y + 2, X + 2), dtype=bool)
    F = np.zeros((Z + 2, Y + 2, X + 2), dtype=F32)
    (x0, y0, z0), (x1, y1, z1) = box if box is not None else ((0, 0, 0), (X - 1, Y - 1, Z - 1))
    x1, y1, z1 = (e - 1 if h == BOX_END else h for h, e in ((x1, X), (y1, Y), (z1, Z)))
    I[z0 + 1:z1 + 2, y0 + 1:y1 + 2, x0 + 1:x1 + 2] = inside[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1]
    F[z0 + 1:z1 + 2, y0 + 1:y1 + 2, x0 + 1:x1 + 2] = f[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1]
    return I, F


def _corner(a, oz, oy, ox):
    """the corner (ox, oy, oz) of every cell: shape (Z + 1, Y + 1, X + 1)"""
    Z, Y, X = (n - 1 for n in a.shape)
    return a[oz:oz + Z, oy:oy + Y, ox:ox + X]


# the 12 edges of a cell in the contract's order: (axis, lower corner offset (x, y, z))
EDGES = ([(0, (0, y, z)) for z in (0, 1) for y in (0, 1)] +      # x-edges by (z, y)
         [(1, (x, 0, z)) for z in (0, 1) for x in (0, 1)] +      # y-edges by (z, x)
         [(2, (x, y, 0)) for y in (0, 1) for x in (0, 1)])       # z-edges by (y, x)
# the cyclic partners (u, v) of an edge's axis: u x v = axis
UV = {0: (1, 2), 1: (2, 0), 2: (0, 1)}


def extract(inside, f, iso, box=None, t_from_far_end=False, unflipped=False, n12=False, no_outside=False):
    """inside: bool (Z, Y, X); f: fp32 (Z, Y, X); returns vertices (N, 3) fp32 in voxel-centre coordinates, cells (N, 3) int32 and
    triangles (M, 3) uint32, vertices in (z, y, x) order of their cells.  The four switches are the negative controls of
    tests/test_mesh_host.py (no_outside: a model without the outside rule -- no quad through a cell that has a phantom corner)."""
    iso = F32(iso)
    I, F = _padded(np.asarray(inside, dtype=bool), np.asarray(f, dtype=F32), box)
    cz, cy, cx = (n - 1 for n in I.shape)
    s = [np.zeros((cz, cy, cx), dtype=F32) for _ in range(3)]
    n = np.zeros((cz, cy, cx), dtype=np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for axis, (ox, oy, oz) in EDGES:
            o0 = (oz, oy, ox)
            o1 = tuple(o + (1 if 2 - k == axis else 0) for k, o in enumerate(o0))
            i0, i1 = _corner(I, *o0), _corner(I, *o1)
            f0, f1 = _corner(F, *o0), _corner(F, *o1)
            cross = i0 != i1
            t = ((iso - f0).astype(F32) / (f1 - f0).astype(F32)).astype(F32)
            if t_from_far_end:
                t = (F32(1) - t).astype(F32)
            t = np.minimum(np.maximum(t, F32(0)), F32(1))
            for a, o in enumerate((ox, oy, oz)):
                add = t if a == axis else np.full_like(t, F32(o))
                s[a] = (s[a] + np.where(cross, add, F32(0))).astype(F32)
            n += cross
    active = n > 0
    zz, yy, xx = np.nonzero(active)   # C order: (z, y, x)
    cells = np.stack([xx, yy, zz], axis=1).astype(np.int32) - 1
    den = np.full(len(xx), F32(12)) if n12 else n[active].astype(F32)
    verts = np.stack([(cells[:, a].astype(F32) + (s[a][active] / den).astype(F32)).astype(F32) for a in range(3)], axis=1)
    index = np.full(active.shape, -1, dtype=np.int64)
    index[active] = np.arange(len(xx))
    tris = []
    for axis in range(3):
        u, v = UV[axis]
        e = [np.array([1 if a == k else 0 for a in range(3)]) for k in range(3)]   # (x, y, z) unit steps
        # edge from padded voxel P to P + e_axis; P ranges over every padded voxel that has a successor
        sl0 = [slice(None)] * 3
        sl1 = [slice(None)] * 3
        sl0[2 - axis] = slice(0, -1)
        sl1[2 - axis] = slice(1, None)
        i0, i1 = I[tuple(sl0)], I[tuple(sl1)]
        pz, py, px = np.nonzero(i0 != i1)
        low_in = i0[pz, py, px]
        p = np.stack([px, py, pz], axis=1)   # padded voxel = cell index + 1 of the cell whose lower corner it is
        # (a crossing edge has an in-volume end, so p[u], p[v] >= 1 and the four cells exist)
        c11 = p
        c00 = p - e[u] - e[v]
        c10 = p - e[v]
        c01 = p - e[u]
        if no_outside:
            top = np.array([cx - 1, cy - 1, cz - 1])
            keep = np.all([((c >= 1) & (c < top)).all(axis=1) for c in (c00, c10, c11, c01)], axis=0)
            c00, c10, c11, c01, low_in = c00[keep], c10[keep], c11[keep], c01[keep], low_in[keep]
        k = [index[c[:, 2], c[:, 1], c[:, 0]] for c in (c00, c10, c11, c01)]
        assert all((q >= 0).all() for q in k)
        fwd = low_in if not unflipped else np.ones_like(low_in)
        b = np.where(fwd, k[1], k[3])
        d = np.where(fwd, k[3], k[1])
        tris.append(np.stack([k[0], b, k[2]], axis=1))
        tris.append(np.stack([k[0], k[2], d], axis=1))
    tris = np.concatenate(tris).astype(np.uint32) if tris else np.zeros((0, 3), np.uint32)
    return verts, cells, tris


def extract_density(d, iso, box=None, **kw):
    d = np.asarray(d, dtype=F32)
    return extract(d >= F32(iso), d, iso, box, **kw)


def extract_segment(mask, box=None, **kw):
    mask = np.asarray(mask, dtype=bool)
    return extract(mask, mask.astype(F32), 0.5, box, **kw)


def counts(inside, box=None):
    """what VxMeshResult reports: vertices, triangles, the inclusive cell bbox (zeros when empty), and the number of cell blocks
    (cells 8B - 1 .. 8B + 6 per axis, B in [0, bricks]) with an active cell, and of cell blocks in all"""
    inside = np.asarray(inside, dtype=bool)
    I, _ = _padded(inside, np.zeros(inside.shape, F32), box)
    c = [_corner(I, oz, oy, ox) for oz in (0, 1) for oy in (0, 1) for ox in (0, 1)]
    anyc, allc = np.logical_or.reduce(c), np.logical_and.reduce(c)
    active = anyc & ~allc
    cross = sum(int((np.take(I, range(0, I.shape[a] - 1), axis=a) != np.take(I, range(1, I.shape[a]), axis=a)).sum())
                for a in range(3))
    zz, yy, xx = np.nonzero(active)
    Z, Y, X = inside.shape
    nbz, nby, nbx = Z // 8 + 1, Y // 8 + 1, X // 8 + 1
    blocks = set(zip((zz // 8).tolist(), (yy // 8).tolist(), (xx // 8).tolist()))   # padded cell index = c + 1 = 8B + local
    out = {"vertices": int(active.sum()), "triangles": 2 * cross, "active_blocks": len(blocks), "blocks": nbz * nby * nbx,
           "bbox_lo": (0, 0, 0), "bbox_hi": (0, 0, 0)}
    if len(xx):
        out["bbox_lo"] = (int(xx.min()) - 1, int(yy.min()) - 1, int(zz.min()) - 1)
        out["bbox_hi"] = (int(xx.max()) - 1, int(yy.max()) - 1, int(zz.max()) - 1)
    return out


def canonical(vertices, cells, triangles):
    """vertices sorted by cell (z, y, x); triangles re-indexed, each rotated (not reflected) to start at its smallest index, rows
    sorted lexicographically"""
    vertices, cells = np.asarray(vertices), np.asarray(cells)
    t = np.asarray(triangles).astype(np.int64).reshape(-1, 3)
    order = np.lexsort((cells[:, 0], cells[:, 1], cells[:, 2])) if len(cells) else np.zeros(0, np.int64)
    inv = np.empty(len(order), dtype=np.int64)
    inv[order] = np.arange(len(order))
    t = inv[t] if len(t) else t
    if len(t):
        k = np.argmin(t, axis=1)
        rows = np.arange(len(t))
        t = np.stack([t[rows, k], t[rows, (k + 1) % 3], t[rows, (k + 2) % 3]], axis=1)
        t = t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]
    return vertices[order], cells[order], t.astype(np.uint32)


# ---- measures on a mesh (float64) -------------------------------------------------------------------------------------------
def area(v, t):
    v = np.asarray(v, dtype=np.float64)
    a, b, c = (v[np.asarray(t)[:, k].astype(np.int64)] for k in range(3))
    return float(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum())


def volume(v, t):
    v = np.asarray(v, dtype=np.float64)
    a, b, c = (v[np.asarray(t)[:, k].astype(np.int64)] for k in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def directed_edges(t):
    t = np.asarray(t).astype(np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def closed_and_oriented(t):
    """every directed edge occurs exactly as often as its reverse"""
    e = directed_edges(t)
    if not len(e):
        return True
    n = int(e.max()) + 1
    fwd = np.unique(e[:, 0] * n + e[:, 1], return_counts=True)
    rev = np.unique(e[:, 1] * n + e[:, 0], return_counts=True)
    return np.array_equal(fwd[0], rev[0]) and np.array_equal(fwd[1], rev[1])


def euler(nv, t):
    e = directed_edges(t)
    und = np.unique(np.sort(e, axis=1), axis=0)
    return int(nv) - len(und) + len(t)
