"""numpy reference of the device post-processing (include/hrseg.h: hrseg_label_components, hrseg_filter_components),
written from the stated semantics alone: breadth-first flood fill in row-major order.  It knows nothing about tiles."""
from collections import deque

import numpy as np


def name2pix(class_map):
    if isinstance(class_map, dict):
        return {k: int(v) for k, v in class_map.items()}
    return {row["class_name"]: int(float(row["pixel_val"])) for row in class_map
            if str(row["pixel_val"]).strip().lower() not in ("", "none", "nan")}


def _offsets(connectivity):
    assert connectivity in (4, 8)
    four = [(-1, 0), (0, -1), (0, 1), (1, 0)]
    return four if connectivity == 4 else four + [(-1, -1), (-1, 1), (1, -1), (1, 1)]


def label(img, group, connectivity):
    """img [H,W] uint8, group: 256 group ids -> (roots, area) int32 [H,W]: per pixel the row-major index of the first pixel
    of its component (equal group id, 4- or 8-connected); the component's pixel count at that first pixel, 0 elsewhere"""
    img = np.asarray(img)
    H, W = img.shape
    # plain lists over the image with a border of one pixel of group -1 (no pixel's group): no bounds tests in the fill
    P = W + 2
    padded = np.full((H + 2, P), -1, dtype=np.int64)
    padded[1:-1, 1:-1] = np.asarray(group, dtype=np.int64)[img]
    g = padded.reshape(-1).tolist()
    seen = [False] * len(g)
    nb = [dy * P + dx for dy, dx in _offsets(connectivity)]
    roots = np.full(H * W, -1, dtype=np.int32)
    area = np.zeros(H * W, dtype=np.int32)
    for y0 in range(H):
        for x0 in range(W):
            s = (y0 + 1) * P + x0 + 1
            if seen[s]:
                continue
            me, members = g[s], [s]                          # scanning in row-major order: the seed is the first pixel
            seen[s] = True
            todo = deque(members)
            while todo:
                i = todo.popleft()
                for d in nb:
                    j = i + d
                    if g[j] == me and not seen[j]:
                        seen[j] = True
                        members.append(j)
                        todo.append(j)
            m = np.asarray(members)
            first = y0 * W + x0
            roots[(m // P - 1) * W + m % P - 1] = first
            area[first] = len(members)
    return roots.reshape(H, W), area.reshape(H, W)


def filter(img, group, rules, connectivity):
    """rules: {group id: (min_area, keep_largest, fill)} with fill 0..255 or -1 (the neighbour rule); groups without an
    entry, and group 255 always, are copied -> (out [H,W] uint8, stats [256,3] int64: found, removed, pixels)"""
    img = np.asarray(img)
    H, W = img.shape
    roots, area = label(img, group, connectivity)
    out = img.copy()
    stats = np.zeros((256, 3), dtype=np.int64)
    flat, oflat, rflat, aflat = img.reshape(-1), out.reshape(-1), roots.reshape(-1), area.reshape(-1)
    firsts = np.nonzero(aflat)[0]
    gid = np.asarray(group, dtype=np.int64)[flat[firsts]]
    best = {}
    for f, g in zip(firsts.tolist(), gid.tolist()):           # ascending first pixel: a tie keeps the earlier one
        if g not in best or aflat[f] > aflat[best[g]]:
            best[g] = f
    for f, g in zip(firsts.tolist(), gid.tolist()):
        stats[g, 0] += 1
        if g == 255 or g not in rules:
            continue
        min_area, keep_largest, fill = rules[g]
        if not (aflat[f] < min_area or (keep_largest and best[g] != f)):
            continue
        if fill < 0:
            if f % W > 0:
                fill = int(flat[f - 1])
            elif f >= W:
                fill = int(flat[f - W])
            else:
                continue                                      # the image's origin: the component stays
        oflat[rflat == f] = fill
        stats[g, 1] += 1
        stats[g, 2] += int(aflat[f])
    return out, stats


def cut_groups(tree, cmap, level):
    """the cut of the tree at `level`: the nodes at depth `level` plus the leaves shallower than it, breadth first ->
    (names of the cut, group [256] uint8: pixel value -> position of its leaf's ancestor-or-self in the cut, 255 for values
    that are no leaf's)"""
    pix = name2pix(cmap)
    names, group = [], np.full(256, 255, dtype=np.uint8)
    frontier = [(name, sub, 0, None) for name, sub in tree.items()]
    while frontier:
        nxt = []
        for name, sub, depth, owner in frontier:
            kids = sub if isinstance(sub, dict) else {}
            if owner is None and (depth == level or not kids):
                owner = len(names)
                names.append(name)
            if not kids:
                group[pix[name]] = owner
            nxt.extend((k, s, depth + 1, owner) for k, s in kids.items())
        frontier = nxt
    return names, group


# ---------------------------------------------------------------------------------------------------------------- patterns
def serpentine(H, W, a=1, b=2):
    """a one-pixel-wide path of value `a` through the whole image: every other row is full, joined alternately at the right
    and the left end; the other pixels hold `b`"""
    m = np.full((H, W), b, dtype=np.uint8)
    m[0::2] = a
    for k, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = a
    return m


def spiral(H, W, a=1, b=2):
    """a one-pixel-wide rectangular spiral of value `a` from the origin inwards, one pixel of `b` between its turns"""
    m = np.full((H, W), b, dtype=np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = a

    def free(yy, xx):
        return 0 <= yy < H and 0 <= xx < W and m[yy, xx] != a

    while True:
        moved = False
        # a step is taken while the pixel ahead is free and the one behind it is not already part of the path
        while free(y + dy, x + dx) and (free(y + 2 * dy, x + 2 * dx) or not (0 <= y + 2 * dy < H and 0 <= x + 2 * dx < W)):
            y, x, moved = y + dy, x + dx, True
            m[y, x] = a
        dy, dx = dx, -dy
        if not moved:
            return m


def checkerboard(H, W, a=1, b=2):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where((yy + xx) % 2 == 0, a, b).astype(np.uint8)


def stripes(H, W, vertical, a=1, b=2):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where((xx if vertical else yy) % 2 == 0, a, b).astype(np.uint8)


def diagonal(H, W, anti, period, a=1, b=2):
    """the lines y - x = 0 (mod period), or x + y = period - 1 (mod period), of `a` on `b`: with the tile height as the
    period they step through tile corners"""
    yy, xx = np.mgrid[0:H, 0:W]
    on = (yy + xx) % period == period - 1 if anti else (yy - xx) % period == 0
    return np.where(on, a, b).astype(np.uint8)


def random_map(rng, H, W, values, p_first=None):
    """values drawn independently; p_first: probability of values[0] (the rest share the remainder)"""
    values = np.asarray(values, dtype=np.uint8)
    if p_first is None:
        return rng.choice(values, size=(H, W))
    p = np.full(len(values), (1.0 - p_first) / max(len(values) - 1, 1))
    p[0] = p_first
    return rng.choice(values, size=(H, W), p=p)
