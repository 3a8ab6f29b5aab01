"""Device consensus: several label maps of the same images -> one map, voted down the class tree, and how far the maps
agree per tree node.  Kernel: csrc/consensus.hip; the semantics are stated once, in include/hrseg.h under "consensus"
(hrseg_consensus_labels), and DESIGN.md section 29.

The members are folds of one model, several teachers or several hedges of one teacher, several annotators, or a test and
its retest.  A vote that fails among the children of a node can still succeed at the node: the result is then the internal
byte that `Data.Hedge` writes and `TargetEncoder(internal_values=...)` / `DeviceAugment(internal_values=...)` read, so a
consensus map plugs into both ends of what exists.  A byte the table does not know (a hedge's reject value, an ignore value,
anything foreign) is an abstention; abstentions count against a node, the denominator of the quorum is always M.

`summary()` turns the integer counters into per-node and per-pair agreement figures on the host, in float64.  The pairwise
`fn`, `fp` and `agreement = 1 - (fn + fp) / 2` are the reference's (AgreementModule.agreement: fn = |A \\ B| / |A|,
fp = |B \\ A| / |B|), with one DELIBERATE DEVIATION: the reference returns agreement 0 when fn == fp == 0, that is, on
perfect agreement; here perfect agreement is 1, and a zero denominator gives NaN.

The tables are built and validated on the host without a GPU; only the call launches.
"""
from __future__ import annotations

import torch

from .. import ops
from .._lib import require_gpu
from .decode import RaggedLabels, build_tables
from .hedge import Hedge
from .score import DeviceScore, build_score_tables


class ConsensusLabels(RaggedLabels):
    """A voted batch (`DeviceConsensus.__call__`): a RaggedLabels whose maps hold leaves' values, internal nodes' bytes
    (`cons.values`) and `cons.none_val`, packed as member 0 was; `support` (packed uint8: the votes of the consensus node, 0
    where the map is none_val) or None; `counts` [R, cells] int64 (device; R = images, or one row of totals): the counters
    of hrseg_consensus_labels for `members` maps per image -- of this call, or of every call it was accumulated over."""

    def __init__(self, labels, desc, desc_host, support, counts, cons, members):
        super().__init__(labels, None, desc, desc_host)
        self.support, self.counts, self.cons, self.members = support, counts, cons, int(members)

    def unpack_support(self):
        """list of H x W uint8 numpy arrays, or None when the call did not keep the support"""
        return None if self.support is None else self._split(self.support.cpu().numpy())

    def _blocks(self):
        """the counters summed over the rows, from ONE device-to-host copy: (ended [N+1], votes [N][M], area [M][N],
        both [P][N], abstain [M]) as lists of ints"""
        M, N = self.members, len(self.cons.node_names)
        host = self.counts.sum(0).cpu().tolist()
        _, first = ops.consensus_cells(N, M)
        P = M * (M - 1) // 2
        ended = host[:N + 1]
        votes = [host[first["votes"] + n * M:first["votes"] + (n + 1) * M] for n in range(N)]
        area = [host[first["area"] + m * N:first["area"] + (m + 1) * N] for m in range(M)]
        both = [host[first["both"] + p * N:first["both"] + (p + 1) * N] for p in range(P)]
        return ended, votes, area, both, host[first["abstain"]:first["abstain"] + M]

    def summary(self):
        """the one host read.  dict(
        members, quorum, pixels;
        nodes {name: dict(ended: pixels whose consensus ended on the node; voters: pixels where at least one member has the
          node on its path; unanimous: the share of those where all M have it; mean_votes: the mean number of members that
          have it, over those pixels; kappa: Fleiss' kappa of "node" against "not node" over the M raters and all pixels, NaN
          for M = 1 or where the chance agreement is 1)};
        none: pixels without a consensus;
        pairs {(i, j), i < j: {name: dict(both, area_i, area_j, dice = 2 both / (area_i + area_j), iou, fn = |i \\ j| / |i|,
          fp = |j \\ i| / |j|, agreement = 1 - (fn + fp) / 2)}};
        abstained [per member]: the share of the pixels where the member's byte names no node).
        Everything follows from the int64 cells in float64; a zero denominator gives NaN."""
        M, names = self.members, self.cons.node_names
        ended, votes, area, both, abstain = self._blocks()
        pixels = sum(ended)
        div = lambda a, b: a / b if b else float("nan")          # noqa: E731
        nodes = {}
        for n, name in enumerate(names):
            voters = sum(votes[n])
            yes = sum((k + 1) * votes[n][k] for k in range(M))
            kappa = float("nan")
            if M > 1 and pixels:
                by_k = [pixels - voters] + votes[n]                  # pixels with exactly k yes votes, k = 0..M
                agree = sum(c * (k * (k - 1) + (M - k) * (M - k - 1)) for k, c in enumerate(by_k)) / (pixels * M * (M - 1))
                p = yes / (pixels * M)
                chance = p * p + (1.0 - p) * (1.0 - p)
                kappa = div(agree - chance, 1.0 - chance)
            nodes[name] = dict(ended=ended[n], voters=voters, unanimous=div(votes[n][M - 1], voters), mean_votes=div(yes, voters),
                               kappa=kappa)
        pairs, p = {}, 0
        for i in range(M):
            for j in range(i + 1, M):
                rows = {}
                for n, name in enumerate(names):
                    b, ai, aj = both[p][n], area[i][n], area[j][n]
                    fn, fp = div(ai - b, ai), div(aj - b, aj)
                    rows[name] = dict(both=b, area_i=ai, area_j=aj, dice=div(2 * b, ai + aj), iou=div(b, ai + aj - b), fn=fn, fp=fp,
                                      agreement=1.0 - (fn + fp) / 2.0)
                pairs[(i, j)] = rows
                p += 1
        return dict(members=M, quorum=self.cons.resolve_quorum(M), pixels=pixels, nodes=nodes, none=ended[len(names)], pairs=pairs,
                    abstained=[div(a, pixels) for a in abstain])

    def pairwise(self, node):
        """the M x M matrices of one node (its name): dict(dice, iou, agreement, fn, fp) of float64 tensors; fn[i][j] =
        |i \\ j| / |i| and fp[i][j] = |j \\ i| / |j| for every ordered pair, the diagonal is a member against itself (NaN
        where the member never names the node)"""
        M = self.members
        n = self.cons.node_names.index(node)
        _, _, area, both, _ = self._blocks()
        pair = {}
        p = 0
        for i in range(M):
            pair[(i, i)] = area[i][n]
            for j in range(i + 1, M):
                pair[(i, j)] = pair[(j, i)] = both[p][n]
                p += 1
        div = lambda a, b: a / b if b else float("nan")          # noqa: E731
        out = {k: torch.empty(M, M, dtype=torch.float64) for k in ("dice", "iou", "agreement", "fn", "fp")}
        for i in range(M):
            for j in range(M):
                b, ai, aj = pair[(i, j)], area[i][n], area[j][n]
                fn, fp = div(ai - b, ai), div(aj - b, aj)
                out["dice"][i, j], out["iou"][i, j] = div(2 * b, ai + aj), div(b, ai + aj - b)
                out["fn"][i, j], out["fp"][i, j], out["agreement"][i, j] = fn, fp, 1.0 - (fn + fp) / 2.0
        return out


class DeviceConsensus:
    """`cons = DeviceConsensus(class_tree, class_map, internal_values=None, ignore_value=None, quorum=None)`;
    `out = cons(members, per_image=False, out=None, want_support=False)` -> ConsensusLabels.
    internal_values: {internal node name: byte}; the internal nodes it does not name get bytes by the rule of `Data.Hedge`
      (its code assigns them).  The full assignment is `cons.values`.
    ignore_value: the byte written where no root reaches the quorum (`cons.none_val`); None: the smallest byte nothing
      else uses.
    quorum: an absolute count with 2 * quorum > M and quorum <= M; None: M // 2 + 1, resolved per call.
    members: a list of RaggedLabels, RaggedBatch (their label side) or (buffer, desc, desc_host) triples.
    out: a ConsensusLabels of an earlier call with the same M, batch size and per_image, whose counters this call adds to
      (the returned object shares them).
    `tables` (Data.score.ScoreTables with the internal bytes), `out_val` per level and channel, `node_names` in the order of
    the counters, `value_names` {byte: node name, none_val: "none"}.  ValueError for everything hrseg_consensus_labels
    refuses, with the nodes' names."""

    def __init__(self, class_tree, class_map, internal_values=None, ignore_value=None, quorum=None):
        self.class_tree, self.class_map = class_tree, class_map
        if ignore_value is not None and not 0 <= int(ignore_value) <= 255:
            raise ValueError(f"DeviceConsensus: ignore value {ignore_value} not in 0..255")
        t = build_tables(class_tree, class_map, 1)
        leaves = {n: int(t.pixel_val[L][c]) for L, names in enumerate(t.names) for c, n in enumerate(names) if not t.n_children[L][c]}
        if ignore_value is not None:
            for name, v in list(leaves.items()) + list((internal_values or {}).items()):
                if int(v) == int(ignore_value):
                    raise ValueError(f"DeviceConsensus: the ignore value and '{name}' share the byte {int(v)}")
        # the bytes of the internal nodes: Hedge's own assignment (all-zero thresholds: a hedge that never stops)
        hedge = Hedge(class_tree, class_map, 0.0, internal_values=internal_values,
                      reject_value=None if ignore_value is None else int(ignore_value))
        self.values = dict(hedge.values)
        if ignore_value is None:
            used = set(leaves.values()) | set(self.values.values())
            free = [v for v in range(256) if v not in used]
            if not free:
                raise ValueError("DeviceConsensus: no unused uint8 value is left for the none value")
            self.none_val = free[0]
        else:
            self.none_val = int(ignore_value)
        self.quorum = None if quorum is None else int(quorum)
        self.tables = build_score_tables(class_tree, class_map, internal_values=self.values)
        self.out_val = [[self.values[n] if n in self.values else leaves[n] for n in names] for names in self.tables.names]
        self.node_names = [n for names in self.tables.names for n in names]
        self.value_names = {v: n for n, v in leaves.items()}
        self.value_names.update({v: n for n, v in self.values.items()})
        self.value_names[self.none_val] = "none"
        self._check_tables()
        self._scorer = None

    @classmethod
    def from_hedge(cls, hedge, quorum=None):
        """the consensus of maps that `hedge` decoded: its internal bytes, and its reject value as the none value (None
        where the hedge rejects nothing)"""
        return cls(hedge.class_tree, hedge.class_map, internal_values=hedge.values,
                   ignore_value=hedge.reject_val if hedge.reject_val >= 0 else None, quorum=quorum)

    def _check_tables(self):
        """path_lut[out_val[n]] ends at node n for every node, and path_lut[none_val] == 0"""
        path = self.tables.path
        for L, names in enumerate(self.tables.names):
            for c, name in enumerate(names):
                e = path[self.out_val[L][c]]
                if (e >> (8 * L)) & 0xFF != c + 1 or e >> (8 * (L + 1)) != 0:
                    raise ValueError(f"DeviceConsensus: the byte {self.out_val[L][c]} of '{name}' does not end at that node in the "
                                     "path table")
        if path[self.none_val] != 0:
            raise ValueError(f"DeviceConsensus: the none value {self.none_val} has a path in the table: it is a node's byte")
        ops.check_consensus(self.tables, self.out_val, self.none_val, 1, 1)

    def resolve_quorum(self, M):
        return M // 2 + 1 if self.quorum is None else self.quorum

    @property
    def scorer(self):
        """a DeviceScore that knows the internal bytes: scores consensus maps against ground truth"""
        if self._scorer is None:
            self._scorer = DeviceScore(self.class_tree, self.class_map, internal_values=self.values)
        return self._scorer

    def __call__(self, members, per_image=False, out=None, want_support=False) -> ConsensusLabels:
        require_gpu()
        triples = []
        for x in members:
            fields = ("label", "ldesc", "ldesc_host") if hasattr(x, "ldesc") else ("labels", "desc", "desc_host")
            triples.append(DeviceScore._triple(x, fields))
        if not triples:
            raise ValueError("consensus_labels: 0 members, supported 1..8")
        device = triples[0][0].device
        triples = [(buf.to(device, non_blocking=True), desc.to(device, non_blocking=True), host) for buf, desc, host in triples]
        M = len(triples)
        if out is not None and out.members != M:
            raise ValueError(f"consensus_labels: out was counted over {out.members} members, this call has {M}")
        labels, support, counts = ops.consensus_labels(triples, self.tables, self.out_val, self.none_val, self.resolve_quorum(M),
                                                       per_image, None if out is None else out.counts, want_support)
        return ConsensusLabels(labels, triples[0][1], triples[0][2], support, counts, self, M)

