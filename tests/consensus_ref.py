"""numpy reference of the device consensus (csrc/consensus.hip, Data/consensus.py): the per-pixel rule of include/hrseg.h
("consensus"), evaluated straight from the class tree and the class map with the tree helpers of tests/score_ref.py.  Pure
integers.  It builds no path table of the product's: a byte is resolved to the set of nodes on its path by walking the
tree, the vote walks the tree from the roots, and every counter is the sum of a boolean mask.

`Nodes` is the tree as the reference sees it: node names in breadth-first order, parents, and per byte the nodes on its
path (leaves' values from the class map, internal nodes' bytes as given).  `vote` is the vectorised reference, `vote_pixel`
the brute-force per-pixel walk that pins it.  The module also holds the case lists of the tests."""
import itertools

import numpy as np

from tests import score_ref as S


class Nodes:
    def __init__(self, tree, class_map, internal_values=None):
        self.levels = S.bfs_levels(tree)
        self.names = [n for names in self.levels for n in names]
        self.level_of = {n: L for L, names in enumerate(self.levels) for n in names}
        self.parent, self.children = {}, {n: [] for n in self.names}

        def walk(node, up):
            for name, sub in node.items():
                self.parent[name] = up
                if up is not None:
                    self.children[up].append(name)
                if isinstance(sub, dict):
                    walk(sub, name)
        walk(tree, None)
        self.roots = [n for n in self.names if self.parent[n] is None]
        pix = S.name2pix(class_map)
        self.byte = {n: int(pix[n]) for n in self.names if not self.children[n]}
        self.byte.update({n: int(v) for n, v in (internal_values or {}).items()})
        self.index = {n: i for i, n in enumerate(self.names)}

    def on_path(self, name):
        """the bytes whose path holds node `name`: its own byte and those of everything below it"""
        out = [self.byte[name]] if name in self.byte else []
        for k in self.children[name]:
            out += self.on_path(k)
        return out

    def descendants(self, name):
        out = []
        for k in self.children[name]:
            out += [k] + self.descendants(k)
        return out


def auto_internal(tree, class_map, given=None, reserved=()):
    """{internal node: byte}: the given ones, the others the smallest bytes nothing else uses, in breadth-first order (the
    rule Data.Hedge states)"""
    nodes = Nodes(tree, class_map)
    given = dict(given or {})
    used = set(nodes.byte.values()) | set(given.values()) | set(reserved)
    free = (v for v in range(256) if v not in used)
    return {n: (given[n] if n in given else next(free)) for n in nodes.names if nodes.children[n]}


def has_masks(members, nodes):
    """[M][N] bool arrays: member m has node n on its path"""
    return [[np.isin(m, nodes.on_path(n)) for n in nodes.names] for m in members]


def vote(members, nodes, none_val, quorum):
    """members: uint8 arrays of one shape -> (labels uint8, support uint8, ended node index int64 (N = none))"""
    has = has_masks(members, nodes)
    N = len(nodes.names)
    votes = [sum(has[m][n].astype(np.int64) for m in range(len(members))) for n in range(N)]
    shape = np.asarray(members[0]).shape
    labels = np.full(shape, none_val, dtype=np.uint8)
    support = np.zeros(shape, dtype=np.uint8)
    ended = np.full(shape, N, dtype=np.int64)

    def descend(name, inside):
        n = nodes.index[name]
        win = inside & (votes[n] >= quorum)
        labels[win] = nodes.byte[name]
        support[win] = votes[n][win]
        ended[win] = n
        for k in nodes.children[name]:
            descend(k, win)
    for r in nodes.roots:
        descend(r, np.ones(shape, dtype=bool))
    return labels, support, ended


def vote_pixel(values, nodes, none_val, quorum):
    """one pixel, brute force: the members' bytes -> (label, support, ended node index)"""
    paths = []
    for v in values:
        path = set()
        for n in nodes.names:
            if nodes.byte.get(n) == int(v):
                while n is not None:
                    path.add(n)
                    n = nodes.parent[n]
        paths.append(path)
    count = lambda n: sum(1 for p in paths if n in p)        # noqa: E731
    here, level = None, nodes.roots
    while True:
        winners = [n for n in level if count(n) >= quorum]
        assert len(winners) <= 1
        if not winners:
            break
        here, level = winners[0], nodes.children[winners[0]]
    if here is None:
        return none_val, 0, len(nodes.names)
    return nodes.byte[here], count(here), nodes.index[here]


def cells(nodes, M):
    """(total, first cell of every block) of a row of counters"""
    N, P = len(nodes.names), M * (M - 1) // 2
    first = dict(ended=0, votes=N + 1, area=N + 1 + N * M, both=N + 1 + 2 * N * M, abstain=N + 1 + 2 * N * M + P * N)
    return first["abstain"] + M, first


def count(members, nodes, none_val, quorum):
    """the row of counters of one image, int64, in the order of include/hrseg.h, + (labels, support)"""
    M, N = len(members), len(nodes.names)
    labels, support, ended = vote(members, nodes, none_val, quorum)
    has = has_masks(members, nodes)
    total, first = cells(nodes, M)
    row = np.zeros(total, dtype=np.int64)
    for n in range(N + 1):
        row[n] = int((ended == n).sum())
    for n in range(N):
        k = sum(has[m][n].astype(np.int64) for m in range(M))
        for j in range(1, M + 1):
            row[first["votes"] + n * M + j - 1] = int((k == j).sum())
        for m in range(M):
            row[first["area"] + m * N + n] = int(has[m][n].sum())
        for p, (i, j) in enumerate(itertools.combinations(range(M), 2)):
            row[first["both"] + p * N + n] = int((has[i][n] & has[j][n]).sum())
    for m in range(M):
        anything = np.zeros(np.asarray(members[m]).shape, dtype=bool)
        for n in range(N):
            anything |= has[m][n]
        row[first["abstain"] + m] = int((~anything).sum())
    return row, labels, support


def count_batch(batches, nodes, none_val, quorum, per_image):
    """batches[m][b]: map b of member m -> (counts [R, cells] int64, [labels per image], [support per image])"""
    rows, labels, support = [], [], []
    for b in range(len(batches[0])):
        r, lab, sup = count([batches[m][b] for m in range(len(batches))], nodes, none_val, quorum)
        rows.append(r)
        labels.append(lab)
        support.append(sup)
    rows = np.stack(rows)
    return (rows if per_image else rows.sum(0, keepdims=True)), labels, support


# ---- trees and maps of the tests
def tl_tree():
    import csv
    import os
    from tests.helpers import DATA, load_tree
    with open(os.path.join(DATA, "class_map.csv")) as f:
        return load_tree("class_tree_tl.json"), list(csv.DictReader(f))


TREES = {"tl": tl_tree, "wide": S.wide_tree, "chain": S.chain_tree, "flat": S.flat_tree, "uniform": S.uniform_tree}
NONE_VAL = 254            # no tree of the tests uses it
FOREIGN = 253             # nor this one: a byte no table knows


def setup(key):
    """(tree, class map, internal bytes, Nodes) of a test tree"""
    tree, cmap = TREES[key]()
    internal = auto_internal(tree, cmap, reserved=(NONE_VAL, FOREIGN))
    return tree, cmap, internal, Nodes(tree, cmap, internal)


def palette(nodes, extra=(NONE_VAL, FOREIGN)):
    """every byte a member map of the tests may hold: leaves, internal nodes, the none / reject byte, a foreign byte"""
    return sorted(set(nodes.byte.values())) + list(extra)


def constant_map(rng, vals, H, W):
    return np.full((H, W), int(rng.choice(vals)), dtype=np.uint8)


def blob_map(rng, vals, H, W, block=5):
    m = rng.choice(np.asarray(vals, dtype=np.uint8), size=((H + block - 1) // block, (W + block - 1) // block))
    return np.ascontiguousarray(np.kron(m, np.ones((block, block), np.uint8))[:H, :W])


def salt_maps(rng, vals, H, W, M):
    """M maps whose member tuple differs between every two neighbouring pixels of the row-major order: member 0 alternates
    between two values, the others are noise"""
    vals = np.asarray(vals, dtype=np.uint8)
    flat = np.arange(H * W)
    first = vals[(flat % 2) * (1 + flat // 2 % (len(vals) - 1))].reshape(H, W) if len(vals) > 1 else np.full((H, W), vals[0])
    return [np.ascontiguousarray(first.astype(np.uint8))] + [rng.choice(vals, size=(H, W)).astype(np.uint8) for _ in range(M - 1)]


REGIMES = ("constant", "blobs", "salt")


def member_maps(rng, regime, vals, H, W, M):
    if regime == "constant":
        return [constant_map(rng, vals, H, W) for _ in range(M)]
    if regime == "blobs":
        return [blob_map(rng, vals, H, W) for _ in range(M)]
    return salt_maps(rng, vals, H, W, M)


MEMBERS = (1, 2, 3, 5, 8)


def quorums(M):
    """both ends of the quorum's range"""
    return sorted({M // 2 + 1, M})
