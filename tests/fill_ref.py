"""Integer restatement of the hole filling of novel views (include/sm_c_api.h "hole filling", DESIGN.md "4n. Hole filling"): the
depth of a novel view from its keys, and the depth-aware push-pull completion -- once vectorised over the image in numpy (fill)
and once as a scalar loop written straight from the rules (fill_scalar).  Every division is a floor division of non-negative
integers.  Both take and return (bgr uint8[..][H][W][3], sem uint8[..][H][W], depth_mm uint16[..][H][W] or None) and, last, the
tally dict(valid, seen_through, filled, left_empty) that sm_fill_stats reports."""
import numpy as np

DEFAULTS = dict(levels=3, depth_tol_256=13, through_count=6, prefer_far=1, min_cover_256=64)
RANGES = dict(levels=(0, 8), depth_tol_256=(0, 255), through_count=(0, 8), prefer_far=(0, 1), min_cover_256=(0, 256))
FAR = 65536                        # the depth of a valid pixel whose depth_mm is 0
NEIGHBOURS = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]
TAP_WEIGHTS = (9, 3, 3, 1)


def params(**over):
    p = dict(DEFAULTS)
    for k, v in over.items():
        if k not in p:
            raise KeyError(k)
        p[k] = int(v)
    return p


def depth_of_d24(d24):
    """depth_mm of a drawn pixel whose key carries d24 (window z = Z / 200 m in 24 bits): 0 beyond 65.535 m"""
    zmm = (np.asarray(d24, np.int64) * 200000 + 8388607) // 16777215
    return np.where(zmm <= 65535, zmm, 0).astype(np.uint16)


def _sizes(w, h, levels):
    out = [(w, h)]
    for _ in range(levels):
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
    return out


def _area(n_cells, size, shift):
    """level-0 pixels inside the image under each of n_cells cells of 2^shift pixels along one axis"""
    X = np.arange(n_cells, dtype=np.int64)
    return np.minimum(size, (X + 1) << shift) - (X << shift)


# ---------------------------------------------------------------------------------------------
# vectorised
# ---------------------------------------------------------------------------------------------
def _see_through(valid, z, tol, T):
    h, w = valid.shape
    vp = np.zeros((h + 2, w + 2), bool)
    zp = np.zeros((h + 2, w + 2), np.int64)
    vp[1:-1, 1:-1] = valid
    zp[1:-1, 1:-1] = z
    nearer = np.zeros((h, w), np.int64)
    for dx, dy in NEIGHBOURS:
        vn = vp[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
        zn = zp[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
        nearer += vn & (zn * (256 + tol) < z * 256)
    return valid & (nearer >= T)


def _pull(lv, w, h, shift, tol, cover):
    """level `shift - 1` (a dict of planes) to level `shift`; w, h: the image's size"""
    v, c, s, z, cnt = lv["v"], lv["c"], lv["s"], lv["z"], lv["cnt"]
    hl, wl = v.shape
    h2, w2 = (hl + 1) // 2, (wl + 1) // 2

    def kids(a):                                     # [h2][w2][4 (dy outer, dx inner)][...]
        pad = np.zeros((h2 * 2, w2 * 2) + a.shape[2:], a.dtype)
        pad[:hl, :wl] = a
        pad = pad.reshape((h2, 2, w2, 2) + a.shape[2:])
        return np.moveaxis(pad, 1, 2).reshape((h2, w2, 4) + a.shape[2:])
    kv, kc, ks, kz, kcnt = kids(v), kids(c), kids(s), kids(z), kids(cnt)
    zmin = np.where(kv, kz, 1 << 40).min(axis=2)
    any_valid = kv.any(axis=2)
    near = kv & (kz * 256 <= zmin[..., None] * (256 + tol))
    n = np.maximum(near.sum(axis=2), 1)
    cc = ((kc * near[..., None]).sum(axis=2) + (n // 2)[..., None]) // n[..., None]
    zz = ((kz * near).sum(axis=2) + n // 2) // n
    first = np.argmax(kv & (kz == zmin[..., None]), axis=2)
    ss = np.take_along_axis(ks, first[..., None], axis=2)[..., 0]
    cn = kcnt.sum(axis=2)
    area = _area(h2, h, shift)[:, None] * _area(w2, w, shift)[None, :]
    return dict(v=any_valid, c=np.where(any_valid[..., None], cc, 0), s=np.where(any_valid, ss, 0), z=np.where(any_valid, zz, 0), cnt=cn,
                may=any_valid & (cn * 256 >= area * cover))


def _push(fine, coarse, tol, prefer_far, level0):
    hl, wl = fine["v"].shape
    hc, wc = coarse["v"].shape
    y, x = np.mgrid[0:hl, 0:wl]
    X, Y = x >> 1, y >> 1
    Xn, Yn = np.where(x & 1, X + 1, X - 1), np.where(y & 1, Y + 1, Y - 1)
    ok, tc, ts, tz = [], [], [], []
    for tx, ty in ((X, Y), (Xn, Y), (X, Yn), (Xn, Yn)):
        inside = (tx >= 0) & (tx < wc) & (ty >= 0) & (ty < hc)
        cx, cy = np.clip(tx, 0, wc - 1), np.clip(ty, 0, hc - 1)
        ok.append(inside & coarse["v"][cy, cx] & coarse["may"][cy, cx])
        tc.append(coarse["c"][cy, cx]); ts.append(coarse["s"][cy, cx]); tz.append(coarse["z"][cy, cx])
    ok, tc, ts, tz = np.stack(ok, -1), np.stack(tc, -2), np.stack(ts, -1), np.stack(tz, -1)     # [h][w][4]...
    wt = np.array(TAP_WEIGHTS, np.int64)
    if prefer_far:
        zmax = np.where(ok, tz, -1).max(axis=-1)
        group = ok & (tz * (256 + tol) >= zmax[..., None] * 256)
    else:
        zmin = np.where(ok, tz, 1 << 40).min(axis=-1)
        group = ok & (tz * 256 <= zmin[..., None] * (256 + tol))
    gw = group * wt
    Wt = np.maximum(gw.sum(axis=-1), 1)
    cc = ((tc * gw[..., None]).sum(axis=-2) + (Wt // 2)[..., None]) // Wt[..., None]
    zz = ((tz * gw).sum(axis=-1) + Wt // 2) // Wt
    first = np.argmax(gw == gw.max(axis=-1)[..., None], axis=-1)          # the weights fall in tap order: the first of the greatest
    ss = np.take_along_axis(ts, first[..., None], axis=-1)[..., 0]
    take = ~fine["v"] & ok.any(axis=-1)
    fine["c"] = np.where(take[..., None], cc, fine["c"])
    fine["z"] = np.where(take, zz, fine["z"])
    fine["s"] = np.where(take, ss, fine["s"])
    fine["v"] = fine["v"] | take
    if not level0:
        fine["may"] = fine["may"] | take
    return take


def _fill_one(bgr, sem, depth, p):
    h, w = sem.shape
    tol, T, L = p["depth_tol_256"], p["through_count"], p["levels"]
    valid = sem != 0
    z = np.where(depth == 0, FAR, depth.astype(np.int64)) if depth is not None else np.full((h, w), FAR, np.int64)
    tally = dict(valid=int(valid.sum()), seen_through=0, filled=0, left_empty=0)
    if T > 0:
        gone = _see_through(valid, z, tol, T)
        tally["seen_through"] = int(gone.sum())
        valid = valid & ~gone
    lv = [dict(v=valid, c=np.where(valid[..., None], bgr, 0).astype(np.int64), s=np.where(valid, sem, 0).astype(np.int64),
               z=np.where(valid, z, 0), cnt=valid.astype(np.int64), may=valid)]
    for l in range(L):
        lv.append(_pull(lv[l], w, h, l + 1, tol, p["min_cover_256"]))
    for l in range(L - 1, -1, -1):
        took = _push(lv[l], lv[l + 1], tol, p["prefer_far"], l == 0)
        if l == 0:
            tally["filled"] = int(took.sum())
    f = lv[0]
    tally["left_empty"] = int((~f["v"]).sum())
    zo = np.where(f["v"] & (f["z"] < FAR), f["z"], 0)
    return (np.where(f["v"][..., None], f["c"], 0).astype(np.uint8), np.where(f["v"], f["s"], 0).astype(np.uint8),
            zo.astype(np.uint16) if depth is not None else None, tally)


def _batched(one, bgr, sem, depth, p):
    bgr, sem = np.asarray(bgr, np.uint8), np.asarray(sem, np.uint8)
    depth = None if depth is None else np.asarray(depth, np.uint16)
    if sem.ndim == 2:
        return one(bgr, sem, depth, p)
    outs = [one(bgr[i], sem[i], None if depth is None else depth[i], p) for i in range(sem.shape[0])]
    tally = {k: sum(o[3][k] for o in outs) for k in ("valid", "seen_through", "filled", "left_empty")}
    return (np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]),
            None if depth is None else np.stack([o[2] for o in outs]), tally)


def fill(bgr, sem, depth=None, p=None):
    return _batched(_fill_one, bgr, sem, depth, params(**(p or {})))


# ---------------------------------------------------------------------------------------------
# the scalar loop
# ---------------------------------------------------------------------------------------------
def _fill_one_scalar(bgr, sem, depth, p):
    h, w = sem.shape
    tol, T, L, cover, far = p["depth_tol_256"], p["through_count"], p["levels"], p["min_cover_256"], p["prefer_far"]
    valid0 = [[int(sem[y, x]) != 0 for x in range(w)] for y in range(h)]
    z0 = [[(FAR if depth is None or int(depth[y, x]) == 0 else int(depth[y, x])) for x in range(w)] for y in range(h)]
    tally = dict(valid=sum(map(sum, valid0)), seen_through=0, filled=0, left_empty=0)
    # a cell: [valid, c0, c1, c2, label, z, cnt, may_fill]
    cur = [[None] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            v = valid0[y][x]
            if v and T > 0:
                nearer = 0
                for dx, dy in NEIGHBOURS:
                    xn, yn = x + dx, y + dy
                    if 0 <= xn < w and 0 <= yn < h and valid0[yn][xn] and z0[yn][xn] * (256 + tol) < z0[y][x] * 256:
                        nearer += 1
                if nearer >= T:
                    v = False
                    tally["seen_through"] += 1
            cur[y][x] = [True, int(bgr[y, x, 0]), int(bgr[y, x, 1]), int(bgr[y, x, 2]), int(sem[y, x]), z0[y][x], 1, True] if v \
                else [False, 0, 0, 0, 0, 0, 0, False]
    levels = [cur]
    sizes = _sizes(w, h, L)
    for l in range(L):
        (wl, hl), (w2, h2) = sizes[l], sizes[l + 1]
        lo, up = levels[l], [[None] * w2 for _ in range(h2)]
        cell = 1 << (l + 1)
        for Y in range(h2):
            for X in range(w2):
                kids = [lo[2 * Y + dy][2 * X + dx] for dy in (0, 1) for dx in (0, 1) if 2 * X + dx < wl and 2 * Y + dy < hl]
                kids_v = [k for k in kids if k[0]]
                cnt = sum(k[6] for k in kids)
                if not kids_v:
                    up[Y][X] = [False, 0, 0, 0, 0, 0, cnt, False]
                    continue
                zmin = min(k[5] for k in kids_v)
                near = [k for k in kids_v if k[5] * 256 <= zmin * (256 + tol)]
                n = len(near)
                c = [(sum(k[1 + i] for k in near) + n // 2) // n for i in range(3)]
                zz = (sum(k[5] for k in near) + n // 2) // n
                s = next(k[4] for k in kids_v if k[5] == zmin)
                area = (min(w, (X + 1) * cell) - X * cell) * (min(h, (Y + 1) * cell) - Y * cell)
                up[Y][X] = [True, c[0], c[1], c[2], s, zz, cnt, cnt * 256 >= area * cover]
        levels.append(up)
    for l in range(L - 1, -1, -1):
        (wl, hl), (w2, h2) = sizes[l], sizes[l + 1]
        lo, up = levels[l], levels[l + 1]
        for y in range(hl):
            for x in range(wl):
                if lo[y][x][0]:
                    continue
                X, Y = x >> 1, y >> 1
                Xn, Yn = (X + 1 if x & 1 else X - 1), (Y + 1 if y & 1 else Y - 1)
                taps = []
                for (tx, ty), wt in zip(((X, Y), (Xn, Y), (X, Yn), (Xn, Yn)), TAP_WEIGHTS):
                    if 0 <= tx < w2 and 0 <= ty < h2 and up[ty][tx][0] and up[ty][tx][7]:
                        taps.append((wt, up[ty][tx]))
                if not taps:
                    continue
                if far:
                    zmax = max(t[5] for _, t in taps)
                    group = [(wt, t) for wt, t in taps if t[5] * (256 + tol) >= zmax * 256]
                else:
                    zmin = min(t[5] for _, t in taps)
                    group = [(wt, t) for wt, t in taps if t[5] * 256 <= zmin * (256 + tol)]
                Wt = sum(wt for wt, _ in group)
                c = [(sum(wt * t[1 + i] for wt, t in group) + Wt // 2) // Wt for i in range(3)]
                zz = (sum(wt * t[5] for wt, t in group) + Wt // 2) // Wt
                wmax = max(wt for wt, _ in group)
                s = next(t[4] for wt, t in group if wt == wmax)
                lo[y][x] = [True, c[0], c[1], c[2], s, zz, 0, l >= 1]
                if l == 0:
                    tally["filled"] += 1
    ob, os_, od = np.zeros((h, w, 3), np.uint8), np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint16)
    for y in range(h):
        for x in range(w):
            k = levels[0][y][x]
            if not k[0]:
                tally["left_empty"] += 1
                continue
            ob[y, x] = k[1:4]
            os_[y, x] = k[4]
            od[y, x] = k[5] if k[5] < FAR else 0
    return ob, os_, (od if depth is not None else None), tally


def fill_scalar(bgr, sem, depth=None, p=None):
    return _batched(_fill_one_scalar, bgr, sem, depth, params(**(p or {})))
