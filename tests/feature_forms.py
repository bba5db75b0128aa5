"""Junction files for the feature build's kernel forms (test_gpu_feature_forms.py; their self-checks, which need no GPU,
run in test_feature_forms_cpu.py).  Not a test module.

Every file begins with a ROSTER: lines that list all samples once, block by block, so that the internal (first-seen) id of
a sample is its place in the roster whatever order the other lines take.  External ids are 1 .. n -- a sample's position
in the "ext" item order is its external id minus one -- dealt to the internal ids at random, ascending inside a roster
block.  Every line has a key of its own: a line's idf depends on its length alone.  All lines pass the threshold of 1.

  Builder / File       lines by column and position inside the column; the arrays prepare_csr and the oracle take
  order probes         cells whose fp32 value depends on the ORDER of their terms (below)
  order_files          groups (a) .. (e) of the order probes
  lengths_file ...     exact line lengths, breaks of the ascent and repeated samples at the hand-over points
  edge_file            one sample count at a form edge, with a few repeat / descending lines and probes
  query_lines          query lines past one tile of query_accumulate_kernel and their fp64 restatement

Order probes.  With coverages below 200 a cell's fp64 sum carries ~30 bits more than its fp32 image: no order of its terms
shows.  A probe cell (sample x, column c) receives, in file order,
    P  +1 * idf_P      a long line (small idf)
    A  +big * idf_A    a short line, big in [2^30, 2^31), key with a positive hash
    B  +1 * idf_B      a long line -- plain, listing x twice, or listing its samples in descending order
    C  -big * idf_A    a line as long as A (the same idf), key with a negative hash in the same column
    S  +1 * idf_S      a long line
and nothing else but its roster entry (coverage 1): the fillers never list a probe sample.  While the sum holds big * idf_A
(2^32 and more) a term is rounded at 2^-20 or coarser, afterwards and before at 2^-52 of its own size: the cell's value
says WHICH terms were added between A and C, to about 2^-21 absolute in a value of about 1 -- eight fp32 ulps.  (Among the
terms between A and C their order does not show: each is rounded to the same grid.  (A + B) + C equals (B + A) + C: taking
A and C behind B would change nothing, so the self-check moves C directly behind A, which takes B out from between them.)
A walk of P A B C S in reverse puts S between instead of behind, passes of lines taken last to first put P and S between.
"""
import functools
import math

import numpy as np

AW_LINES, AW_TILE, AW_THREADS = 32, 4096, 256      # accumulate_piece_kernel (with an item order)
ACC_LINES, ACC_TILE, ACC_PFD = 256, 8192, 4        # accumulate_kernel (without)
QA_TILE = 4096                                     # query_accumulate_kernel
KINDS = ("plain", "twice", "desc")


class File(object):
    """lines: (key, external sample ids, coverages); order: the file's lines; alt: the same with every probe's C directly
    behind its A.  probes: dict(tag, col, xs, at) -- at: the position of P, A, B, C, S among their column's lines."""

    def __init__(self, D, n, sample_count, lines, order, alt, ext, probes):
        self.D, self.n, self.sample_count, self.threshold = D, n, sample_count, 1
        self.lines, self.order, self.alt, self.ext, self.probes = lines, order, alt, ext, probes
        self.iid = np.empty(n + 1, np.int64)               # internal id of an external id
        self.iid[ext] = np.arange(n)
        self._ref = None

    def arrays(self, order=None):
        """keys, row_ptr, samples, coverages of the lines in `order` (default: the file's)."""
        order = self.order if order is None else order
        keys = [self.lines[j][0] for j in order]
        rp = np.zeros(len(order) + 1, np.int64)
        np.cumsum([len(self.lines[j][1]) for j in order], out=rp[1:])
        s = np.concatenate([self.lines[j][1] for j in order]).astype(np.int64)
        c = np.concatenate([self.lines[j][2] for j in order]).astype(np.int64)
        return keys, rp, s, c

    def oracle(self, order=None):
        """The oracle's result for the lines in `order`, its rows in the order of the FILE's internal ids."""
        from oracle import capi
        keys, rp, s, c = self.arrays(order)
        buf, off = capi.pack_keys(keys)
        ref = capi.index_features(buf, off, rp, s, c, self.sample_count, self.threshold, self.D, max_items=self.n)
        if order is not None:
            ref["X"] = ref["X"][np.argsort(ref["ext_ids"])][self.ext - 1]
        return ref

    def reference(self):
        if self._ref is None:
            self._ref = self.oracle()
            assert self._ref["n_items"] == self.n and self._ref["ext_ids"].tolist() == self.ext.tolist()
        return self._ref

    def cells(self, tag=None):
        """(internal id, column) of the probe cells."""
        return [(int(self.iid[x]), p["col"]) for p in self.probes if tag in (None, p["tag"]) for x in p["xs"]]

    def tags(self):
        return sorted(set(p["tag"] for p in self.probes))

    def changed(self, X, tag=None):
        """How many probe cells of X differ from the reference's, as bytes."""
        R = self.reference()["X"].view(np.uint32)
        X = np.ascontiguousarray(X).view(np.uint32)
        return sum(1 for i, c in self.cells(tag) if X[i, c] != R[i, c])

    def column_lines(self):
        """Per column, the file's lines (positions in `order`) in file order."""
        from oracle import capi
        buf, off = capi.pack_keys([self.lines[j][0] for j in self.order])
        col = capi.hash_col_sign(buf, off, self.D)[1]
        return [np.nonzero(col == c)[0] for c in range(self.D)]

    def reordered(self, within):
        """The file's order with every column's lines permuted by `within` (positions 0 .. m - 1 -> their new order);
        the lines of other columns keep their places."""
        order = np.array(self.order)
        for at in self.column_lines():
            order[at] = order[at[within(len(at))]]
        return order.tolist()


def reverse_inside_passes(lines):
    """A column's lines walked in reverse inside every pass of `lines` lines."""
    return lambda m: np.concatenate([np.arange(min(l0 + lines, m) - 1, l0 - 1, -1) for l0 in range(0, m, lines)])


def passes_last_to_first(lines):
    return lambda m: np.concatenate([np.arange(l0, min(l0 + lines, m)) for l0 in range(0, m, lines)][::-1])


def check_probes(f):
    """The generator's own check: per tag (planted, kept) -- kept: the cells whose bytes change when every probe's C moves
    directly behind its A.  At least a quarter of all planted cells and 8 of every group must distinguish."""
    alt = f.oracle(f.alt)["X"]
    out = {t: (len(f.cells(t)), f.changed(alt, t)) for t in f.tags()}
    planted, kept = sum(v[0] for v in out.values()), sum(v[1] for v in out.values())
    assert 4 * kept >= planted, out
    assert all(v[1] >= 8 for v in out.values()), out
    return out


class Builder(object):
    def __init__(self, D, n, seed, block, n_lines, sample_count=None):
        from oracle import capi
        self.D, self.n, self.rng = D, n, np.random.default_rng(seed)
        self.sample_count = int(sample_count or n + n // 2)
        cand = ["chr%d %d %d" % (1 + i % 22, 10**4 + i, 10**6 + 3 * i + seed) for i in range(4 * n_lines + 64 * D)]
        buf, off = capi.pack_keys(cand)
        _, col, sign = capi.hash_col_sign(buf, off, D)
        self.pool = {}
        for k, c, sg in zip(cand, col.tolist(), sign.tolist()):
            self.pool.setdefault((c, sg), []).append(k)
        self.ext = self.rng.permutation(n).astype(np.int64) + 1
        for b0 in range(0, n, block):
            self.ext[b0:b0 + block].sort()
        self.block = block
        self.n_roster = (n + block - 1) // block
        self.base = [len(range(c, self.n_roster, D)) for c in range(D)]   # roster lines at the head of every column
        self.cols = [[] for _ in range(D)]
        self.lines, self.probes = [], []
        self.free = np.arange(1, n + 1, dtype=np.int64)
        self.reserved = np.zeros(0, np.int64)
        self.next_col = 0

    def reserve(self, xs):
        """The probe samples: no filler lists them, the roster gives them coverage 1."""
        self.reserved = np.unique(np.asarray(xs, np.int64))
        self.free = np.setdiff1d(np.arange(1, self.n + 1, dtype=np.int64), self.reserved)
        return self.reserved

    def key(self, col, sign=None):
        if sign is None:
            sign = 1 if len(self.pool.get((col, 1), ())) >= len(self.pool.get((col, -1), ())) else -1
        return self.pool[(col, sign)].pop()

    def add(self, samples, cov=None, col=None, sign=None):
        """One more line at the end of column `col` (default: the columns in turn); returns its place in the column."""
        if col is None:
            col, self.next_col = self.next_col, (self.next_col + 1) % self.D
        samples = np.asarray(samples, np.int64)
        cov = self.rng.integers(1, 200, len(samples)) if cov is None else np.asarray(cov, np.int64)
        assert len(cov) == len(samples) > 0 and samples.min() >= 1 and samples.max() <= self.n
        self.lines.append((self.key(col, sign), samples, cov))
        self.cols[col].append(len(self.lines) - 1)
        return self.base[col] + len(self.cols[col]) - 1

    def some(self, k, lo=1, hi=None):
        """k free samples with external ids in [lo, hi], ascending."""
        free = self.free[(self.free >= lo) & (self.free <= (hi or self.n))]
        return np.sort(self.rng.choice(free, k, replace=False))

    def filler(self, col, upto, lo, hi):
        while self.base[col] + len(self.cols[col]) < upto:
            self.add(self.some(int(self.rng.integers(lo, hi))), col=col)

    def probe(self, col, tag, xs, at, long_lo, long_hi, kind="plain", short=6, lo=20, hi=60):
        """P A B C S for the samples xs at the places `at` (ascending) of column col; fillers in between."""
        xs = np.sort(np.asarray(xs, np.int64))
        assert kind in KINDS and np.isin(xs, self.reserved).all() and list(at) == sorted(set(at))
        big = self.rng.integers(2**30, 2**31, len(xs))
        lens = self.rng.choice(np.arange(long_lo, long_hi), 3, replace=False)   # three different idf
        got = []
        for role, where in zip("PABCS", at):
            self.filler(col, where, lo, hi)
            if role in "AC":
                s = np.concatenate([xs, self.some(short)])
                c = np.concatenate([big, self.rng.integers(1, 200, short)])
                sign = 1 if role == "A" else -1
            else:
                others = self.some(int(lens["PBS".index(role)]))
                s = np.concatenate([xs, others])
                c = np.concatenate([np.ones(len(xs), np.int64), self.rng.integers(1, 200, len(others))])
                sign = None
            o = np.argsort(s, kind="stable")
            s, c = s[o], c[o]
            if role == "B" and kind == "twice":
                s, c = np.concatenate([s, xs]), np.concatenate([c, np.ones(len(xs), np.int64)])
            if role == "B" and kind == "desc":
                s, c = s[::-1], c[::-1]
            assert self.add(s, c, col=col, sign=sign) == where, (tag, role, where)
            got.append(len(self.lines) - 1)
        self.probes.append(dict(tag=tag, col=col, xs=xs, at=tuple(at), line_a=got[1], line_c=got[3]))

    def finish(self):
        roster_cov = self.rng.integers(1, 200, self.n)
        roster_cov[np.isin(self.ext, self.reserved)] = 1
        first = len(self.lines)
        for b in range(self.n_roster):
            at = slice(b * self.block, min(self.n, (b + 1) * self.block))
            self.lines.append((self.key(b % self.D), self.ext[at], roster_cov[at]))
        order = list(range(first, len(self.lines)))
        for i in range(max(len(c) for c in self.cols)):
            order += [c[i] for c in self.cols if i < len(c)]
        alt = list(order)
        for p in self.probes:
            alt.remove(p["line_c"])
            alt.insert(alt.index(p["line_a"]) + 1, p["line_c"])
        return File(self.D, self.n, self.sample_count, self.lines, order, alt, self.ext, self.probes)


# ------------------------------------------------------------------------------------------------ A: order probes

def _small(seed, n_lines):
    b = Builder(8, 300, seed, 300, n_lines)
    return b, b.reserve(b.rng.choice(300, 16, replace=False) + 1)


@functools.lru_cache(maxsize=None)
def order_file(group):
    """Group (a) .. (e) of the order probes; the file has passed check_probes."""
    if group == "a":
        # with the item order: A, B and C inside one pass of AW_LINES lines of their column, and in three different ones
        b, xs = _small(101, 8 * 170)
        for col in range(8):
            b.probe(col, "a-same", xs[:4], (34, 39, 46, 54, 61), 150, 240)
            b.probe(col, "a-three", xs[4:8], (70, 71, 110, 150, 151), 150, 240)
            b.probe(col, "a-edge", xs[8:12], (158, 159, 160, 161, 162), 150, 240)      # A | B C across a pass edge
        for p in b.probes:
            pa, pb, pc = [x // AW_LINES for x in p["at"][1:4]]
            assert {"a-same": pa == pb == pc, "a-three": pa < pb < pc and p["at"][3] - p["at"][1] > 2 * AW_LINES,
                    "a-edge": pa + 1 == pb == pc}[p["tag"]]
    elif group == "b":
        # without: the same for passes of ACC_LINES lines (columns of 560 lines), inside one turn of the ACC_PFD ring, and
        # across the hand-over between two passes
        b, xs = _small(102, 8 * 570)
        for col in range(8):
            b.probe(col, "b-ring", xs[:4], (20, 21, 22, 23, 24) if col % 2 else (20, 21, 23, 25, 26), 150, 240)
            if col % 2:
                b.probe(col, "b-three", xs[4:10], (30, 100, 330, 530, 540), 150, 240)
            else:
                b.probe(col, "b-edge", xs[4:10], (253, 254, 256, 257, 258) if col % 4 else (252, 255, 256, 257, 258), 150, 240)
                b.probe(col, "b-same", xs[10:16], (260, 270, 300, 400, 420), 150, 240)
            b.filler(col, 560, 20, 60)
        for p in b.probes:
            pa, pb, pc = [x // ACC_LINES for x in p["at"][1:4]]
            assert {"b-same": pa == pb == pc == 1, "b-three": (pa, pb, pc) == (0, 1, 2), "b-edge": pa == 0 and pb == pc == 1,
                    "b-ring": p["at"][3] - p["at"][1] <= ACC_PFD}[p["tag"]]
    elif group in ("c", "d"):
        # B lists x twice (flag 2, or the serial replay) / lists its samples in descending order (flag 1, or the ordinary path)
        b, xs = _small(103 if group == "c" else 104, 8 * 60)
        for col in range(8):
            b.probe(col, group, xs[:4], (3, 6, 9, 12, 15), 150, 240, kind="twice" if group == "c" else "desc")
            b.probe(col, group + "-near", xs[4:8], (20, 21, 22, 23, 24), 150, 240, kind="twice" if group == "c" else "desc")
            b.filler(col, 40, 20, 60)
    elif group == "e":
        # 8200 samples: three tiles of the item order, the last of 8 positions; x at the order positions 4095 | 4096 (in the
        # reversed order too), at the internal ids 8191 | 8192, and at both ends of either numbering
        n = 8200
        b = Builder(8, n, 105, 1025, 8 * 20)
        at = [AW_TILE - 1, AW_TILE, n - AW_TILE, n - 1 - AW_TILE, 0, n - 1]                  # order positions
        xs = b.reserve([p + 1 for p in at] + b.ext[[ACC_TILE - 1, ACC_TILE, 0, n - 1]].tolist())
        assert len(xs) == 10
        for col in range(8):
            b.probe(col, "e", xs, (3, 4, 5, 6, 7), 2500, 3500, lo=100, hi=3000)
            b.filler(col, 12, 100, 3000)
    else:
        raise ValueError(group)
    f = b.finish()
    f.kept = check_probes(f)
    return f


# --------------------------------------------------------------------------- B: exact lengths and hand-over points

EXACT_LENGTHS = (1, 63, 64, 65, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537, 2047, 2048, 2049, 2048 + 513,
                 2048 + 1025, 2048 + 1537, 4096, 4097)
PLANT_LENGTHS = (130, 2048, 2049 + 600)


def _with_repeats(a, pairs):
    """The ascending list a with, for (i, k) in pairs (ascending k), entry k a repeat of entry i of the RESULT."""
    out = list(a)
    for i, k in pairs:
        assert i < k <= len(out)
        out.insert(k, out[i])
    return np.array(out, np.int64)


def repeat_plants(L, wide=False):
    """Named (entry, entry) pairs of one repeated sample for a line of L entries.  wide: for the workgroup-per-line flag
    kernel (1024 threads, entries t and t + 1024 with one thread).
    Two lanes that meet the same cell in ONE instruction lose a term for certain when the line's flag says "no repeat";
    the same entry pair held by one thread (5 | 5 + 2048, 0 | 1024) or by two waves is added correctly, or mostly so, even
    then -- so beside every pair that the flag kernels must SEE there is one of neighbouring entries they see the same way."""
    out = {"63|64": [(63, 64)], "0|last": [(0, L - 1)], "two in 0..63": [(10, 11), (40, 50)]}
    if L > 5 + 2048 + 1:
        out["5|5+2048"] = [(5, 5 + 2048)]
        out["2053|2054"] = [(2053, 2054)]
    if wide:
        out["0|1023"] = [(0, 1023)]
        if L > 1026:
            out["0|1024"] = [(0, 1024)]
            out["1024|1025"] = [(1024, 1025)]
            out["3|1024"] = [(3, 1024)]
    return {k: v for k, v in out.items() if all(b < L for _, b in v)}


def _break_at(a, k):
    """The ascending list a, its largest value moved to entry k - 1: entry k lies below entry k - 1, all else ascends."""
    a = list(a)
    return np.array(a[:k - 1] + [a[-1]] + a[k - 1:-1], np.int64)


@functools.lru_cache(maxsize=None)
def lengths_file():
    """4300 samples at D = 24 (two tiles of the item order, the second of 204 positions); see the module's head."""
    n = 4300
    b = Builder(24, n, 201, 1075, 200)
    b.names = []

    def add(name, s):
        b.names.append(name)
        b.add(s)
    for L in EXACT_LENGTHS:
        add("len %d" % L, b.some(L))
    for L in PLANT_LENGTHS:
        for k in (64, 2048):
            if k < L:
                # entries k - 1 | k on opposite sides of order position 4096 (external id 4097)
                a = np.concatenate([b.some(L - 1, hi=AW_TILE), b.some(1, lo=AW_TILE + 1)])
                s = _break_at(a, k)
                assert s[k] < s[k - 1] and s[k - 1] > AW_TILE >= s[k] and (np.diff(np.delete(s, k - 1)) > 0).all()
                add("len %d break at %d" % (L, k), s)
        for name, pairs in repeat_plants(L).items():
            s = _with_repeats(b.some(L - len(pairs)), pairs)
            assert len(s) == L and all(s[i] == s[k] for i, k in pairs) and len(np.unique(s)) == L - len(pairs)
            add("len %d repeat %s" % (L, name), s)
    for k in (AW_THREADS, AW_THREADS + 1, 3 * AW_THREADS + 7):      # entries of ONE tile of the order in a line
        add("%d entries in tile 0" % k, np.concatenate([b.some(k, hi=AW_TILE), b.some(10, lo=AW_TILE + 1)]))
    add("descending", b.some(700)[::-1])
    add("shuffled", b.rng.permutation(b.some(2500)))
    f = b.finish()
    f.names = b.names
    return f


@functools.lru_cache(maxsize=None)
def wide_file():
    """66 000 samples at D = 8 -- the duplicate flags come from line_flags_kernel, a workgroup of 1024 threads per line --
    with lines of 1023, 1024, 1025 and 2100 entries and the repeat plants."""
    n = 66000
    b = Builder(8, n, 202, 2200, 200)
    b.names = []
    for L in (1023, 1024, 1025, 2100):
        b.names.append("len %d" % L)
        b.add(b.some(L))
        for name, pairs in repeat_plants(L, wide=True).items():
            s = _with_repeats(b.some(L - len(pairs)), pairs)
            assert len(s) == L and all(s[i] == s[k] for i, k in pairs)
            b.names.append("len %d repeat %s" % (L, name))
            b.add(s)
    b.add(b.some(1500)[::-1])
    f = b.finish()
    f.names = b.names
    return f


# ------------------------------------------------------------------------------------------ C: sample-count edges

EDGE_COUNTS = (65536, 65537, 524288, 524320, 1 << 20, (1 << 20) + 32)


@functools.lru_cache(maxsize=2)
def edge_file(n):
    """n samples at D = 8 in roster lines of 3500, and per column a probe (its samples at both ends of either numbering and
    at a tile edge), a line that repeats samples, a descending and a shuffled one, all of a few thousand samples from the
    whole range."""
    b = Builder(8, n, 300 + n % 1000, 3500, 400)
    xs = b.reserve([1, n, AW_TILE, AW_TILE + 1] + b.ext[[0, n - 1, n - 64, ACC_TILE - 1, ACC_TILE]].tolist())
    for col in range(8):
        b.probe(col, "edge", xs, (b.base[col], b.base[col] + 1, b.base[col] + 2, b.base[col] + 3, b.base[col] + 4), 2000, 3000,
                kind=KINDS[col % 3], lo=2000, hi=3000)
        b.add(_with_repeats(b.some(2500), [(10, 11), (5, 2053), (0, 2300)]), col=col)
        b.add(b.some(2100)[::-1], col=col)
        b.add(b.rng.permutation(b.some(2100)), col=col)
    f = b.finish()
    f.kept = check_probes(f)
    return f


# ------------------------------------------------------------------------------------------------- E: query rows

def query_lines(nq, D, seed=401, n_keys=600, sample_count=20000):
    """About 600 query lines, a key of the vocabulary each (all different): dict(prep, vocab, want64) -- prep as
    ParsedLines.from_arrays takes it, vocab: key -> frequency, want64: the rows restated in numpy fp64, per line in file
    order R[ids, col] = R[ids, col] + cov * (sign * w) with one rounding per multiply and per add."""
    from oracle import capi
    rng = np.random.default_rng(seed + nq)
    keys = ["chr%d %d %d" % (1 + j % 22, 5000 + 13 * j, 9000 + 17 * j) for j in range(n_keys)]
    df = rng.integers(1, 4000, n_keys)
    lens = rng.integers(1, 300, n_keys)
    lens[:8] = (1, 255, 256, 257, 3000, 3000, 2900, 1)
    lens = np.minimum(lens, nq)
    lists = []
    for j, L in enumerate(lens.tolist()):
        if j == 4 and nq > QA_TILE:                      # all of it in the second tile (what there is of it)
            s = QA_TILE + rng.choice(min(nq, 2 * QA_TILE) - QA_TILE, min(L, min(nq, 2 * QA_TILE) - QA_TILE), replace=False)
        elif j == 5 and nq > QA_TILE:                    # astride 4095 | 4096, in the line's own (shuffled) order
            s = rng.permutation(np.union1d(rng.choice(nq, L - 2, replace=False), [QA_TILE - 1, QA_TILE]))
        elif j == 7:
            s = np.array([nq - 1])
        else:
            s = rng.choice(nq, L, replace=False)
            if j % 3:
                s = np.sort(s)
        lists.append(s.astype(np.int64))
    order = np.concatenate([[0, 1, 2, 3], rng.permutation(np.arange(4, n_keys))])     # the long lines anywhere in their columns
    keys, df, lists = [keys[j] for j in order], df[order], [lists[j] for j in order]
    rp, ids, cov = [0], [], []
    key_off = np.zeros(n_keys + 1, np.int64)
    np.cumsum([len(k) for k in keys], out=key_off[1:])
    for s in lists:
        ids.append(s)
        cov.append(rng.integers(1, 200, len(s)))
        rp.append(rp[-1] + len(s))
    ids, cov = np.concatenate(ids), np.concatenate(cov)
    prep = dict(key_bytes=np.frombuffer("".join(keys).encode(), np.uint8), key_off=key_off, row_ptr=np.array(rp, np.int64),
                ids=ids, cov=cov, idf=np.zeros(n_keys), ext_ids=np.arange(nq, dtype=np.int64))
    buf, off = capi.pack_keys(keys)
    _, col, sign = capi.hash_col_sign(buf, off, D)
    w = np.array([math.log(float(sample_count) / float(f)) for f in df.tolist()])
    R = np.zeros((nq, D), np.float64)
    for j in range(n_keys):
        at = ids[rp[j]:rp[j + 1]]
        R[at, col[j]] = R[at, col[j]] + cov[rp[j]:rp[j + 1]].astype(np.float64) * (float(sign[j]) * w[j])
    return dict(prep=prep, vocab={k: int(f) for k, f in zip(keys, df.tolist())}, want64=R, keys=keys, df=df, rp=rp,
                sample_count=sample_count)


def finalize_row(q, lines, D):
    """Row q of query_lines' rows from the oracle's finalize_query: the lines that list q, in file order."""
    from oracle import capi
    rp, ids, cov = lines["rp"], lines["prep"]["ids"], lines["prep"]["cov"]
    keys, cs, fs = [], [], []
    for j, k in enumerate(lines["keys"]):
        at = np.nonzero(ids[rp[j]:rp[j + 1]] == q)[0]
        if len(at):
            keys.append(k)
            cs.append(int(cov[rp[j] + at[0]]))
            fs.append(int(lines["df"][j]))
    if not keys:
        return np.zeros(D)
    return capi.finalize_query(keys, cs, fs, lines["sample_count"], D)
