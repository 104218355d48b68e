"""A map set turned into a triangle mesh, restated (sm_mesh_maps; include/sm_c_api.h, "meshing"; DESIGN.md "4u. Meshing").  This
file is the contract the HIP path is compared with, bit for bit.  Integers are int64 (nothing below leaves its range), the stated
fp64 and fp32 operations are numpy's of that type, one at a time.

A set is a list of (global id, record) pairs; a record is 12 float32 (48 bytes): x y z conf | colour word, -, t0, t1 | nx ny nz radius.

Grid.      The simplification's: V = (voxel_mm * 65536 + 500) // 1000; X[k] = floor((float64(p[k]) - float64(origin[k])) * 65536.0);
           cell[k] = X[k] // V (floor division); off[k] = X[k] - cell[k] * V; and its regular-record test.
Records.   LOOSE: not regular.  SKIPPED: regular, bit c & 31 of class_mask[c >> 5] clear (c = colour word >> 24).  OUTSIDE: some
           cell[k] outside [-65536 + reach, 65535 - reach].  USED: every other record.
Cells.     Per cell of USED records: n, SW, SP[3], SN[3], SC[3] (the simplification's weight w and integers) and cmin = the minimum
           of (id << 8) | c.  A cell with n < min_records does not exist.  mp[k] = (SP[k] + SW // 2) // SW; n_c = merged_normal(SN), a
           cell for which that fails has no plane: it exists, but adds nothing to F.
Lattice.   l is an integer triple at l * V.  Inner cells: l - b, b in {0, 1}^3.  Outer cells: l - 2 <= c <= l + 1.  reach 1: l is
           sampled iff an inner cell exists.  reach 2: iff an outer cell exists.  Contributors: the inner cells that exist; if there
           is none (reach 2), the outer cells that exist.  In ascending lexicographic order of c - l, in fp64:
             F += float64(SW_c) * ((n0 * e0 + n1 * e1) + n2 * e2),  e[k] = float64((l[k] - c[k]) * V - mp_c[k]),  F begins as 0.0
           (cells without a plane left out); W, NS[3], CS[3] = the integer sums of SW_c, SN_c, SC_c and cmin = the minimum of cmin_c
           over ALL contributors.  l is inside iff F < 0.
Cubes.     The cube at l (corners l + b) is meshed iff its eight corners are sampled.  Six Kuhn tetrahedra, one per permutation
           (a, b, c) of the axes in lexicographic order: t0 = l, t1 = l + e_a, t2 = l + e_a + e_b, t3 = l + (1, 1, 1); t2 and t3
           exchanged for an odd permutation.
Faces.     Of a tetrahedron by its inside corners: none with 0 or 4.  One corner i unlike the other three j < k < l: k and l
           exchanged if i is odd ((i, j, k, l) is then an odd permutation); the triangle (v_ij, v_ik, v_il), reversed (first and last
           exchanged) if the lone corner is the outside one.  Two inside i < j, two outside k < l: k and l exchanged if (i, j, k, l)
           is odd; (v_ik, v_il, v_jl), then (v_ik, v_jl, v_jk).  Each triangle rotated so that its smallest index comes first.
Vertices.  v_ab lies on the edge from lattice point a to b = a + d, d in {0, 1}^3 \\ {0}; a owns it; kind = d0 + 2 d1 + 4 d2.  It
           exists iff a face refers to it.  t = A / (A - B), A = F_a * float64(W_b), B = F_b * float64(W_a);
           pos[k] = float32(float64(origin[k]) + (float64(a[k] * V) + t * float64(d[k] * V)) * 2^-16);
           normal = merged_normal(NS_a + NS_b) or (0, 0, 0); channel k = ((CS_a + CS_b)[k] + (W_a + W_b) // 2) // (W_a + W_b);
           class = the low byte of min(cmin_a, cmin_b).
Order.     Vertices ascending by (owner, kind), owners in lexicographic order of l, x major.  Faces ascending by (cube's l,
           tetrahedron, triangle).

Worked by hand, voxel_mm 1000 (V = 65536), origin 0: one record at (.5, .5, .5) with normal +z.  Cell (0, 0, 0), X = 32768, so
mp = (32768, 32768, 32768) and F(l) = w * (l_z * 65536 - 32768): l is inside iff l_z <= 0, and t = 1/2 on every cut edge.
  reach 1: the 8 lattice points {0, 1}^3, one cube.  Cut edges: those with d_z = 1 -- 4 upright edges, 4 upright face diagonals, the
  body diagonal: 9 vertices at z = 0.5 exactly.  Four tetrahedra have one or three corners inside (one triangle), two have two (two
  triangles): 8 faces, a disc (V - E + F = 1), every face normal +z.
  reach 2: the 64 lattice points {-1..2}^3 (the layers l_z = -1 and 2 have no inner cell and take the outer one: the same sign), 27
  cubes, the 9 of the layer l_z = 0 cut: 49 vertices, 72 faces."""

import numpy as np

import segment_ref as sg

F32, F64 = np.float32, np.float64
DEFAULTS = dict(voxel_mm=100, reach=2, min_records=1, class_mask=(0xFFFFFFFF,) * 8, max_cells=1 << 24, origin=(0.0, 0.0, 0.0))
VERTEX = np.dtype([("pos", "<f4", 3), ("normal", "<f4", 3), ("colour", "<u4")])
KINDS = ("USED", "SKIPPED", "LOOSE", "OUTSIDE")
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
PERM_ODD = (False, True, True, False, False, True)


class Capacity(Exception):
    """more cells than max_cells"""


def cell_edge(voxel_mm):
    return (int(voxel_mm) * 65536 + 500) // 1000


def tet_corners(t):
    """the four corners of tetrahedron t as cube-corner masks b0 + 2 b1 + 4 b2"""
    a, b, _ = PERMS[t]
    c = [0, 1 << a, (1 << a) | (1 << b), 7]
    if PERM_ODD[t]:
        c[2], c[3] = c[3], c[2]
    return c


def _odd(p):
    return sum(1 for i in range(4) for j in range(i + 1, 4) if p[i] > p[j]) % 2 == 1


def tet_faces(mask):
    """the triangles of a tetrahedron whose corners with their bit in `mask` are inside: a list of three edges (x, y) each, x and y
    tetrahedron corners"""
    ins = [i for i in range(4) if mask >> i & 1]
    outs = [i for i in range(4) if not mask >> i & 1]
    if len(ins) in (0, 4):
        return []
    if len(ins) == 2:
        i, j = ins
        k, l = outs
        if _odd((i, j, k, l)):
            k, l = l, k
        return [[(i, k), (i, l), (j, l)], [(i, k), (j, l), (j, k)]]
    i = ins[0] if len(ins) == 1 else outs[0]
    j, k, l = [x for x in range(4) if x != i]
    if _odd((i, j, k, l)):
        k, l = l, k
    tri = [(i, j), (i, k), (i, l)]
    return [tri[::-1]] if len(ins) == 3 else [tri]


def _pack(u):
    """(u per axis, 17 bits each, x highest): monotone in the lexicographic order of u"""
    return (u[..., 0] << 34) | (u[..., 1] << 17) | u[..., 2]


def _bit_length(v):
    bits, v = np.zeros(len(v), np.int64), v.copy()
    while (v > 0).any():
        bits += v > 0
        v >>= 1
    return bits


def merged_normal(sn):
    """the simplification's merged normal of int64[n, 3] sums -> (float32[n, 3], ok); rows that fail are (0, 0, 0)"""
    sn = np.asarray(sn, np.int64).reshape(-1, 3)
    sh = np.maximum(0, _bit_length(np.abs(sn).max(axis=1, initial=0)) - 24)
    f = (sn >> sh[:, None]).astype(F32)                                   # (>> floors, as the device's arithmetic shift does)
    ok = ~(f == 0).all(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        ln = np.sqrt((f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) + f[:, 2] * f[:, 2])
        n = f / ln[:, None]
    assert n.dtype == F32
    n[~ok] = 0
    return n, ok


def classify(rows, voxel_mm, origin):
    """(regular, cell int64[n, 3], off int64[n, 3], class) per row; cell and off are 0 where the row is loose"""
    rows = np.asarray(rows, F32).reshape(-1, 12)
    ok, cell, cls = sg.cells(rows, voxel_mm, origin)
    V = cell_edge(voxel_mm)
    off = np.zeros((len(rows), 3), np.int64)
    for k in range(3):
        d = rows[:, k].astype(F64) - F64(F32(origin[k]))
        X = np.floor(np.where(ok, d, 0.0) * 65536.0).astype(np.int64)
        off[:, k] = np.where(ok, X - cell[:, k] * V, 0)
    return ok, cell, off, cls


def _lookup(keys, want, valid):
    """index of want in the sorted keys, -1 where it is absent or not valid"""
    if len(keys) == 0:
        return np.full(want.shape, -1, np.int64)
    at = np.minimum(np.searchsorted(keys, want), len(keys) - 1)
    return np.where(valid & (keys[at] == want), at, -1)


def mesh(rows, ids=None, voxel_mm=100, reach=2, min_records=1, class_mask=(0xFFFFFFFF,) * 8, max_cells=1 << 24, origin=(0.0, 0.0, 0.0)):
    """-> dict(vertices: VERTEX rows, faces: uint32[m, 3], info).  ids: the rows' global ids (default: their positions)"""
    assert reach in (1, 2) and min_records >= 1
    rows = np.asarray(rows, F32).reshape(-1, 12)
    n = len(rows)
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    V = cell_edge(voxel_mm)
    ok, cell, off, cls = classify(rows, voxel_mm, origin)
    words = np.asarray(class_mask, np.uint64)
    takes_part = ((words[cls >> 5] >> (cls & 31).astype(np.uint64)) & np.uint64(1)).astype(bool)
    inside_grid = ((cell >= -65536 + reach) & (cell <= 65535 - reach)).all(axis=1)
    kind = np.where(~ok, 2, np.where(~takes_part, 1, np.where(~inside_grid, 3, 0)))
    counts = [int((kind == k).sum()) for k in range(4)]

    # ---- cells
    idx = np.flatnonzero(kind == 0)
    r = rows[idx]
    t = r[:, 3] * F32(16.0)
    with np.errstate(invalid="ignore"):
        w = np.where(t >= 255, 255, np.maximum(1, t.astype(np.int64))).astype(np.int64)
    col = np.ascontiguousarray(r[:, 4]).view(np.uint32).astype(np.int64)
    ni = np.clip(np.floor(r[:, 8:11] * F32(16384.0) + F32(0.5)), F32(-4194304.0), F32(4194304.0)).astype(np.int64)
    ckeys, node_of = np.unique(_pack(cell[idx] + 65536), return_inverse=True)
    C = len(ckeys)
    if C > max_cells:
        raise Capacity(C)
    cn = np.bincount(node_of, minlength=C).astype(np.int64)
    SW = np.zeros(C, np.int64)
    SP, SN, SC = np.zeros((C, 3), np.int64), np.zeros((C, 3), np.int64), np.zeros((C, 3), np.int64)
    cmin = np.full(C, np.iinfo(np.int64).max, np.int64)
    np.add.at(SW, node_of, w)
    np.add.at(SP, node_of, w[:, None] * off[idx])
    np.add.at(SN, node_of, w[:, None] * ni)
    np.add.at(SC, node_of, w[:, None] * np.stack([(col >> (8 * k)) & 255 for k in range(3)], axis=1))
    np.minimum.at(cmin, node_of, (ids[idx] << 8) | cls[idx])
    ccell = np.zeros((C, 3), np.int64)
    ccell[node_of] = cell[idx]
    exists = cn >= min_records
    ckeys, ccell, SW, SP, SN, SC, cmin = ckeys[exists], ccell[exists], SW[exists], SP[exists], SN[exists], SC[exists], cmin[exists]
    C = len(ckeys)
    mp = (SP + (SW // 2)[:, None]) // np.maximum(SW, 1)[:, None]
    cnorm, plane = merged_normal(SN)

    # ---- lattice points, in key order
    span = range(-1, 3) if reach == 2 else range(0, 2)
    offs = np.asarray([(x, y, z) for x in span for y in span for z in span], np.int64)
    lat = np.unique(_pack((ccell[:, None, :] + offs[None, :, :]).reshape(-1, 3) + 65536)) if C else np.zeros(0, np.int64)
    L = len(lat)
    l = np.stack([(lat >> 34) & 0x1FFFF, (lat >> 17) & 0x1FFFF, lat & 0x1FFFF], axis=1) - 65536

    def contributors(sel, deltas):
        """for the lattice points sel: per delta (c - l) in order, the index of the cell or -1"""
        out = []
        for d in deltas:
            c = l[sel] + np.asarray(d, np.int64)
            valid = ((c >= -65536) & (c <= 65535)).all(axis=1)            # a cell outside the grid does not exist
            out.append(_lookup(ckeys, _pack(np.where(valid[:, None], c, 0) + 65536), valid))
        return out

    F, W = np.zeros(L, F64), np.zeros(L, np.int64)
    NS, CS = np.zeros((L, 3), np.int64), np.zeros((L, 3), np.int64)
    lmin = np.full(L, np.iinfo(np.int64).max, np.int64)

    def accumulate(sel, deltas):
        hits = contributors(sel, deltas)
        for d, at in zip(deltas, hits):
            hit = at >= 0
            c = np.where(hit, at, 0)
            e = ((-np.asarray(d, np.int64))[None, :] * V - mp[c]).astype(F64)
            nn = cnorm[c].astype(F64)
            term = SW[c].astype(F64) * ((nn[:, 0] * e[:, 0] + nn[:, 1] * e[:, 1]) + nn[:, 2] * e[:, 2])
            F[sel] = np.where(hit & plane[c], F[sel] + term, F[sel])
            W[sel] += np.where(hit, SW[c], 0)
            NS[sel] += np.where(hit[:, None], SN[c], 0)
            CS[sel] += np.where(hit[:, None], SC[c], 0)
            lmin[sel] = np.where(hit, np.minimum(lmin[sel], cmin[c]), lmin[sel])
        return np.stack(hits, axis=1).max(axis=1, initial=-1) >= 0 if len(sel) else np.zeros(0, bool)

    inner = [(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (-1, 0)]
    every = np.arange(L)
    if C:
        has_inner = accumulate(every, inner)
        rest = every[~has_inner]
        if reach == 2 and len(rest):
            assert accumulate(rest, [(x, y, z) for x in range(-2, 2) for y in range(-2, 2) for z in range(-2, 2)]).all()
        else:
            assert has_inner.all()
        assert (W > 0).all()
    inside = F < 0

    # ---- cubes, tetrahedra, faces
    corner = []
    for b in range(8):
        c = l + np.asarray([b & 1, b >> 1 & 1, b >> 2 & 1], np.int64)
        valid = (c <= 65535).all(axis=1)
        corner.append(_lookup(lat, _pack(np.where(valid[:, None], c, 0) + 65536), valid))
    corner = np.stack(corner, axis=1) if L else np.zeros((0, 8), np.int64)
    cube = np.flatnonzero((corner >= 0).all(axis=1))
    tri_key, tri_edges = [], []                                             # per triangle: (cube, tet, tri), its three (owner, kind)
    for t in range(6):
        tc = tet_corners(t)
        m4 = sum(inside[corner[cube, tc[i]]].astype(np.int64) << i for i in range(4)) if len(cube) else np.zeros(0, np.int64)
        for mask in range(1, 15):
            at = cube[m4 == mask]
            if not len(at):
                continue
            for j, tri in enumerate(tet_faces(mask)):
                edges = []
                for x, y in tri:
                    a, b = min(tc[x], tc[y]), max(tc[x], tc[y])
                    assert a & b == a and a != b                            # the lower end's corner is contained in the upper's
                    edges.append(corner[at, a] * 8 + (a ^ b))
                tri_key.append(np.stack([at, np.full(len(at), t), np.full(len(at), j)], axis=1))
                tri_edges.append(np.stack(edges, axis=1))
    if tri_key:
        tri_key, tri_edges = np.concatenate(tri_key), np.concatenate(tri_edges)
        order = np.lexsort((tri_key[:, 2], tri_key[:, 1], tri_key[:, 0]))
        tri_edges = tri_edges[order]
        vkeys, inv = np.unique(tri_edges.reshape(-1), return_inverse=True)
        faces = inv.reshape(-1, 3).astype(np.int64)
        first = faces.argmin(axis=1)
        faces = np.stack([faces[np.arange(len(faces)), (first + k) % 3] for k in range(3)], axis=1).astype(np.uint32)
    else:
        vkeys, faces = np.zeros(0, np.int64), np.zeros((0, 3), np.uint32)

    # ---- vertices
    a, dk = vkeys >> 3, vkeys & 7
    d = np.stack([dk & 1, dk >> 1 & 1, dk >> 2 & 1], axis=1)
    b = corner[a, dk] if len(a) else a
    vertices = np.zeros(len(vkeys), VERTEX)
    if len(vkeys):
        A, B = F[a] * W[b].astype(F64), F[b] * W[a].astype(F64)
        t = A / (A - B)
        o = np.asarray([F64(F32(v)) for v in origin], F64)
        vertices["pos"] = (o[None, :] + ((l[a] * V).astype(F64) + t[:, None] * (d * V).astype(F64)) * F64(1.0 / 65536.0)).astype(F32)
        vertices["normal"] = merged_normal(NS[a] + NS[b])[0]
        ws = W[a] + W[b]
        ch = (CS[a] + CS[b] + (ws // 2)[:, None]) // ws[:, None]
        vertices["colour"] = ((np.minimum(lmin[a], lmin[b]) & 255) << 24 | ch[:, 2] << 16 | ch[:, 1] << 8 | ch[:, 0]).astype(np.uint32)
    info = dict(records=n, counts_by_kind=counts, cells=C, lattice_points=L, cubes=len(cube), vertices=len(vertices), faces=len(faces))
    return dict(vertices=vertices, faces=faces, info=info)


def mesh_set(parts, **params):
    """the mesh of a set given as its parts in order (files, then the live model): ids run on across them"""
    parts = [np.asarray(p, F32).reshape(-1, 12) for p in parts]
    return mesh(np.concatenate(parts) if parts else np.zeros((0, 12), F32), **params)


PLY_HEADER = ("ply\nformat binary_little_endian 1.0\ncomment surfelmapping mesh\nelement vertex %d\nproperty float x\nproperty float y\n"
              "property float z\nproperty float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\n"
              "property uchar blue\nproperty uchar class\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n")
PLY_VERTEX = np.dtype([("pos", "<f4", 3), ("normal", "<f4", 3), ("rgbc", "u1", 4)])
PLY_FACE = np.dtype([("n", "u1"), ("v", "<i4", 3)])


def ply_bytes(vertices, faces):
    """the file sm_mesh_maps writes: red, green, blue are bytes 2, 1, 0 of the colour word, class its byte 3"""
    v = np.zeros(len(vertices), PLY_VERTEX)
    v["pos"], v["normal"] = vertices["pos"], vertices["normal"]
    c = vertices["colour"]
    v["rgbc"] = np.stack([c >> 16 & 255, c >> 8 & 255, c & 255, c >> 24], axis=1).astype(np.uint8) if len(c) else np.zeros((0, 4), np.uint8)
    f = np.zeros(len(faces), PLY_FACE)
    f["n"], f["v"] = 3, np.asarray(faces, np.uint32).reshape(-1, 3).view(np.int32)
    return (PLY_HEADER % (len(v), len(f))).encode() + v.tobytes() + f.tobytes()


# ---- what a test measures of a mesh
def edges_of(faces):
    """directed edges int64[3 m, 2]"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def topology(faces, n_vertices):
    """dict(open_edges, bad_edges (undirected edges not in exactly two faces), repeated (directed edges used more than once), euler)"""
    e = edges_of(faces)
    und = np.sort(e, axis=1)
    _, ucount = np.unique(und, axis=0, return_counts=True)
    _, dcount = np.unique(e, axis=0, return_counts=True)
    return dict(open_edges=int((ucount == 1).sum()), bad_edges=int((ucount != 2).sum()), repeated=int((dcount > 1).sum()),
                euler=n_vertices - len(ucount) + len(np.asarray(faces).reshape(-1, 3)))


def signed_volume(vertices, faces):
    p = vertices["pos"].astype(F64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return float(np.einsum("ij,ij->i", p[f[:, 0]], np.cross(p[f[:, 1]], p[f[:, 2]])).sum() / 6.0)


def face_normals(vertices, faces):
    p = vertices["pos"].astype(F64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
