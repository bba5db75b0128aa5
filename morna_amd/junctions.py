"""Host side of `morna junctions`: the junctions-by-sample store and the splice-file writer.

Stands in for commanderson/morna morna.py:221-341 (update_junction_dbs and its 100 sqlite shards) and 1486-1638 (the
retention step and the output loop of the `junctions` subcommand).  The store -- for every sample id of any line of the
indexed intropolis file, its ascending (line number, coverage) list -- is built, kept and filtered by libmorna_hip.so
(csrc/jstore.hip); this module marshals numpy buffers, computes min_count with the reference's own expression and
writes the text.

    store = JunctionStore.build(ParsedLines(path, sample_count=n, sample_threshold=0))
    store.save(basename + ".junc.mor")
    kept = JunctionStore.load(basename + ".junc.mor").retain([[sample ids in rank order], ...], 0.05, 5)

Pooled samples (create_supersample.py of the reference's tests/): `JunctionStore.pool` sums the rows of
groups of samples on the GPU, `write_supersample_files` writes the "chrom start end sum" files of that script.

Depth thinning: `JunctionStore.thin` gives store rows with every read kept with one probability, by a
counter-based integer hash on the GPU; `parse_downsample` reads the rates of `--downsample`.
"""
import ctypes as C
import gzip
import re
from math import ceil, isfinite

import numpy as np

from ._lib import check, lib, ptr, read_stats

MAX_RESULTS = 64        # found_in is one 64-bit word per line (morna_jstore_retain)
STORE_SUFFIX = ".junc.mor"
WEIGHTS_SUFFIX = ".jw.mor"      # the line weights of the unhashed search (save_weights)
WEIGHTS_MAGIC = b"MORNAJW1"
MAX_NEAREST = 1024              # neighbours per query of the unhashed search (MORNA_JNEAREST_MAX_K)
MAX_GRID = 15                   # coverage thresholds of one recovery call (morna_jstore_recovery)
MAX_PREFIXES = 8                # list lengths of one recovery sweep (morna_jstore_recovery_sweep)
MAX_RATES = 16                  # rates of one --downsample
KEEP_ALL = 2**32                # the threshold that keeps every read (morna_jstore_thin)
MAX_THIN_COVERAGE = 2**24       # the largest coverage of a row that can be thinned
DEFAULT_DOWNSAMPLE_SEED = 8675309
DEFAULT_RECOVERY_GRID = "0,.05,.1,.2,.3,.5,.75,1:1,2,3,5,10,20,50,1000"
RECOVERY_COLUMNS = ("frequency_filter", "coverage_filter", "min_count", "retrieved", "true_positive", "false_positive",
                    "false_negative", "precision", "recall", "fscore")


def parse_junction_filter(text):
    """--junction-filter "<frequency>,<coverage>" as (float, int) (morna.py:1487-1489); ValueError otherwise."""
    parts = str(text).split(",")
    if len(parts) != 2:
        raise ValueError("--junction-filter takes two parts separated by a comma, such as .05,5 (got %r)" % (text,))
    return float(parts[0]), int(parts[1])


def min_count(frequency_filter, n_results):
    """Results that must hold a junction for the frequency filter to keep it (morna.py:1551)."""
    return int(ceil(frequency_filter * n_results))


def parse_recovery_grid(text=None):
    """--grid "<f1>,<f2>,...:<c1>,<c2>,..." as (frequencies, coverages); None is the default grid.  The frequencies are
    kept as given, in any number and order, each the text float() reads (so that a table prints them as they were
    typed); the coverages are integers, sorted and de-duplicated, at most 15.  ValueError otherwise."""
    text = DEFAULT_RECOVERY_GRID if text is None else str(text)
    halves = text.split(":")
    if len(halves) != 2:
        raise ValueError("--grid takes frequencies and coverages separated by a colon, such as 0,.05,.5:1,5,50 (got %r)" % (text,))
    frequencies = [t.strip() for t in halves[0].split(",")]
    for t in frequencies:
        if not isfinite(float(t)):                             # (float() raises on anything that is no number)
            raise ValueError("--grid: a frequency must be a finite number (got %r)" % (text,))
    coverages = sorted(set(int(t) for t in halves[1].split(",")))
    if len(coverages) > MAX_GRID:
        raise ValueError("--grid holds %d distinct coverages: one recovery call takes at most %d" % (len(coverages), MAX_GRID))
    return frequencies, coverages


def parse_results_sweep(text):
    """--results-sweep "<p1>,<p2>,...": the result counts to tabulate, as integers sorted and de-duplicated; each in 1 to
    64, at most 8 distinct ones.  ValueError otherwise."""
    values = sorted(set(int(t) for t in str(text).split(",")))             # (int() raises on "", "1.5" and "a")
    for p in values:
        if p < 1 or p > MAX_RESULTS:
            raise ValueError("--results-sweep: %d is outside 1 to %d, the results a list holds" % (p, MAX_RESULTS))
    if len(values) > MAX_PREFIXES:
        raise ValueError("--results-sweep holds %d distinct values: one sweep takes at most %d" % (len(values), MAX_PREFIXES))
    return values


def parse_downsample(text):
    """--downsample "<p1>,<p2>,...": 1 to 16 distinct rates, each a float in [0, 1], in the order typed.  Returns (the rates
    as typed, the thresholds int(round(rate * 2^32)) of morna_jstore_thin).  ValueError otherwise."""
    typed = [t.strip() for t in str(text).split(",")]
    if len(typed) > MAX_RATES:
        raise ValueError("--downsample holds %d rates: one run takes at most %d" % (len(typed), MAX_RATES))
    rates = []
    for t in typed:
        rate = float(t)                                        # (float() raises on "", "a" and "1/2")
        if not 0.0 <= rate <= 1.0:                             # (nan fails both comparisons)
            raise ValueError("--downsample: a rate is a number in [0, 1] (got %r)" % (t,))
        if rate in rates:
            raise ValueError("--downsample names the rate %r twice" % (t,))
        rates.append(rate)
    return typed, [int(round(rate * 4294967296.0)) for rate in rates]


def _ratio(a, b):
    return float(a) / float(b) if b else float("nan")


def _recovery_row(frequency, coverage, mc, retrieved, tp, true):
    """One row of a recovery table from its three counts (the expressions of junction_recovery_performance.py:320-330,
    with nan where that script would divide by zero)."""
    p, r = _ratio(tp, retrieved), _ratio(tp, true)
    f = 2 * p * r / (p + r) if p + r > 0 else float("nan")
    return dict(zip(RECOVERY_COLUMNS, (frequency, coverage, mc, retrieved, tp, retrieved - tp, true - tp, p, r, f)))


def recovery_rows(hist_q, n_results, frequencies, coverages, extra_true=0):
    """The recovery table of one query from its histogram hist_q[2][65][B + 1] (JunctionStore.recovery made over the grid
    `coverages`, B of them ascending): one dict of RECOVERY_COLUMNS per (frequency, coverage), frequency-major in the
    order given.  A line of class (cnt, b) is retrieved under (f, coverages[i]) when cnt >= 1 and (cnt >= min_count(f,
    n_results) or b > i) -- what retain(f, coverages[i]) keeps.  extra_true: true junctions that are no line of the file
    and so can never be retrieved; they add to `true` and false_negative.  Pure host code."""
    h = np.asarray(hist_q, np.int64)
    if h.ndim != 3 or h.shape[0] != 2 or h.shape[2] != len(coverages) + 1:
        raise ValueError("recovery_rows takes the histogram of one query, [2][%d][%d] for %d coverages (got shape %r)"
                         % (h.shape[1] if h.ndim == 3 else MAX_RESULTS + 1, len(coverages) + 1, len(coverages), h.shape))
    true = int(h[1].sum()) + int(extra_true)
    cnt = np.arange(h.shape[1])[:, None]
    b = np.arange(h.shape[2])[None, :]
    rows = []
    for frequency in frequencies:
        mc = min_count(float(frequency), n_results)
        for i, coverage in enumerate(coverages):
            kept = (cnt >= 1) & ((cnt >= mc) | (b > i))
            rows.append(_recovery_row(frequency, coverage, mc, int(h[:, kept].sum()), int(h[1][kept].sum()), true))
    return rows


def sum_recovery_rows(tables):
    """The micro-average of several queries' tables (recovery_rows of the same grid): the counts summed cell by cell and
    the ratios taken from the sums; min_count, which differs from query to query, is "-"."""
    tables = list(tables)
    out = []
    for cell in zip(*tables):
        retrieved = sum(r["retrieved"] for r in cell)
        tp = sum(r["true_positive"] for r in cell)
        true = sum(r["true_positive"] + r["false_negative"] for r in cell)
        out.append(_recovery_row(cell[0]["frequency_filter"], cell[0]["coverage_filter"], "-", retrieved, tp, true))
    return out


def format_recovery_rows(rows):
    """The column line and one tab-separated line per row: floats as %.12f, or nan."""
    def cell(v):
        if isinstance(v, float):
            return "nan" if v != v else "%.12f" % v
        return str(v)
    return "\t".join(RECOVERY_COLUMNS) + "\n" + "".join("\t".join(cell(r[c]) for c in RECOVERY_COLUMNS) + "\n" for r in rows)


class Retained(object):
    """The junctions retained for one result list: lines (ascending line numbers, int32 array), found_in (per line, the
    ranks of the results that hold it, ascending) and coverages (per line, their coverages in that order)."""

    def __init__(self, lines, masks, cov_ptr, cov):
        self.lines = lines
        self.masks = masks
        self._cov_ptr, self._cov = cov_ptr, cov

    def __len__(self):
        return len(self.lines)

    @property
    def found_in(self):
        return [[r for r in range(MAX_RESULTS) if (m >> r) & 1] for m in self.masks.tolist()]

    @property
    def coverages(self):
        p = self._cov_ptr
        return [self._cov[p[i]:p[i + 1]].tolist() for i in range(len(self.lines))]


class Pooled(object):
    """A group of samples summed (JunctionStore.pool): lines (the line numbers at least one member holds, ascending, int32),
    sums (the members' summed coverage of each, int64) and holders (the members that hold it, int32)."""

    def __init__(self, lines, sums, holders):
        self.lines, self.sums, self.holders = lines, sums, holders

    def __len__(self):
        return len(self.lines)


class Thinned(object):
    """A store row at a fraction of its depth (JunctionStore.thin): lines (the line numbers that keep at least one read,
    ascending, int32) and cov (the reads each keeps, int32)."""

    def __init__(self, lines, cov):
        self.lines, self.cov = lines, cov

    def __len__(self):
        return len(self.lines)


class Explained(object):
    """One (query, result) pair of JunctionStore.explain: the sums pq, pp, qq, pp_shared, qq_shared and
    the unhashed distance (fp64, in the contract's order), the counts shared, n_q, n_r, and the top list -- lines (int32),
    terms (fp64, descending; equal terms by ascending line) and cov_r (the result's coverages, int32)."""
    SUMS = ("pq", "pp", "qq", "pp_shared", "qq_shared", "distance")
    COUNTS = ("shared", "n_q", "n_r")

    def __init__(self, sums, counts, lines, terms, cov_r):
        self.sums, self.counts = np.asarray(sums, np.float64), np.asarray(counts, np.int64)
        for name, x in zip(self.SUMS, self.sums.tolist()):
            setattr(self, name, x)
        for name, n in zip(self.COUNTS, self.counts.tolist()):
            setattr(self, name, n)
        self.lines, self.terms, self.cov_r = lines, terms, cov_r

    @property
    def query_outside(self):
        """The share of the query's squared weight on lines the result lacks: 1 - qq_shared / qq (nan for qq = 0)."""
        return 1.0 - self.qq_shared / self.qq if self.qq > 0 else float("nan")

    @property
    def result_outside(self):
        """The share of the result's squared weight on lines the query lacks: 1 - pp_shared / pp (nan for pp = 0)."""
        return 1.0 - self.pp_shared / self.pp if self.pp > 0 else float("nan")


def lost_lines(row_lines, row_cov, thinned_lines, min_coverage=1):
    """The truth of `recovery --downsample --lost-only`: the lines of a sample's full row covered at least min_coverage
    times that its thinned row does not hold -- what the shallow sequencing lost -- ascending, int32.  Pure host code."""
    row_lines, row_cov = np.asarray(row_lines, np.int64), np.asarray(row_cov, np.int64)
    full = row_lines[row_cov >= int(min_coverage)]
    return np.setdiff1d(full, np.asarray(thinned_lines, np.int64)).astype(np.int32)


def view(pp, ctype, count):
    """A copy of `count` elements of library-owned memory."""
    if count == 0 or not pp.value:
        return np.zeros(0, np.dtype(ctype))
    return np.ctypeslib.as_array(C.cast(pp, C.POINTER(ctype)), shape=(count,)).copy()


def _clamp62(x):
    """int(x) held inside [-2^62, 2^62]: every threshold the library takes as an int64."""
    return min(max(int(x), -2**62), 2**62)


def _pack_lists(lists, what, limit=MAX_RESULTS):
    """Result lists (external sample ids in rank order) as (res [nq][k] int64, n_res [nq] int32, k), k the longest
    list's length, at least 1; past `limit` (64) results ValueError, `what` the words for who takes no more."""
    lists = [[int(s) for s in lst] for lst in lists]
    k = max([len(lst) for lst in lists] + [1])
    if k > limit:
        raise ValueError(("a result list holds %d results: " + what) % (k, limit))
    res = np.zeros((len(lists), k), np.int64)
    n_res = np.zeros(len(lists), np.int32)
    for q, lst in enumerate(lists):
        res[q, :len(lst)] = lst
        n_res[q] = len(lst)
    return res, n_res, k


def _pack_queries(queries):
    """Unhashed queries, a (lines, coverages) pair each, as the CSR the library takes: (q_ptr int64 [nq + 1], q_line int32,
    q_cov int32); ValueError for a pair that is not two 1-d arrays of one length."""
    queries = [(np.ascontiguousarray(l, np.int32), np.ascontiguousarray(c, np.int32)) for l, c in queries]
    for l, c in queries:
        if l.ndim != 1 or l.shape != c.shape:
            raise ValueError("an unhashed query is a pair of 1-d arrays of one length: lines and coverages")
    q_ptr = np.zeros(len(queries) + 1, np.int64)
    np.cumsum([len(l) for l, _ in queries], out=q_ptr[1:])
    q_line = np.concatenate([l for l, _ in queries] + [np.zeros(0, np.int32)]).astype(np.int32)
    q_cov = np.concatenate([c for _, c in queries] + [np.zeros(0, np.int32)]).astype(np.int32)
    return q_ptr, q_line, q_cov


# the doubles of every morna_jstore_*_stats call, in the order of the C array (the *_stats methods say what they mean)
NEAREST_STATS = (("candidates", int), ("max_candidates", int), ("passes", int), ("kernel_ms", float), ("bytes", int),
                 ("queries_per_pass", int), ("norms_ms", float), ("window", float))
EXPLAIN_STATS = (("pairs", int), ("entries", int), ("passes", int), ("kernel_ms", float), ("bytes", int), ("queries_per_pass", int))
RECOVERY_STATS = (("kernel_ms", float), ("bytes", int), ("workgroups", int))
POOL_STATS = (("kernel_ms", float), ("bytes_read", int), ("bytes_written", int), ("workgroups", int))
THIN_STATS = (("kernel_ms", float), ("bytes_read", int), ("bytes_written", int), ("draws", int), ("workgroups", int))
HASH_ROWS_STATS = (("kernel_ms", float), ("bytes_read", int), ("bytes_written", int), ("workgroups", int))


class JunctionStore(object):
    """A junction store held by the library (morna_jstore)."""

    def __init__(self, _ptr):
        self._p = _ptr
        counts = np.zeros(3, np.int64)
        check(lib().morna_jstore_counts(self._p, ptr(counts)))
        self.n_samples, self.nnz, self.n_lines = [int(x) for x in counts]

    @classmethod
    def build(cls, parsed, device=0):
        """From a ParsedLines of the whole file with sample_threshold=0 (every line kept), on the GPU."""
        p = C.c_void_p()
        check(lib().morna_jstore_build(int(device), parsed._p, C.byref(p)))
        return cls(p)

    @classmethod
    def from_arrays(cls, ext_ids, ptr_, line, cov, n_lines, device=0):
        a = [np.ascontiguousarray(x, t) for x, t in ((ext_ids, np.int64), (ptr_, np.int64), (line, np.int32), (cov, np.int32))]
        if len(a[1]) != len(a[0]) + 1 or len(a[2]) != len(a[3]) or (len(a[1]) and a[1][-1] != len(a[2])):
            raise ValueError("junction store arrays: ptr must hold one more entry than ext_ids and end at the length of line / cov")
        p = C.c_void_p()
        check(lib().morna_jstore_from_arrays(int(device), ptr(a[0]), len(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3]), int(n_lines),
                                             C.byref(p)))
        return cls(p)

    @classmethod
    def load(cls, path, device=0):
        p = C.c_void_p()
        check(lib().morna_jstore_load(str(path).encode(), int(device), C.byref(p)))
        return cls(p)

    def save(self, path):
        check(lib().morna_jstore_save(self._p, str(path).encode()))

    def __del__(self):
        p = getattr(self, "_p", None)
        if p is not None and p.value:
            try:
                lib().morna_jstore_free(p)
            except Exception:                          # interpreter shutting down
                pass
            self._p = None

    def sample_ids(self):
        out = np.zeros(self.n_samples, np.int64)
        check(lib().morna_jstore_samples(self._p, ptr(out)))
        return out

    def sample(self, ext_id):
        """(line numbers, coverages) of one sample; IndexError for an id the store lacks."""
        n = C.c_int64()
        check(lib().morna_jstore_sample(self._p, int(ext_id), C.byref(n), None, None))
        line, cov = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32)
        check(lib().morna_jstore_sample(self._p, int(ext_id), C.byref(n), ptr(line), ptr(cov)))
        return line, cov

    def timers(self):
        """{"build": (ms, bytes), "retain": (ms, bytes)}: kernel time of the build and of the last retain."""
        ms, nbytes = np.zeros(2, np.float64), np.zeros(2, np.int64)
        check(lib().morna_jstore_timers(self._p, ptr(ms), ptr(nbytes)))
        return {"build": (float(ms[0]), int(nbytes[0])), "retain": (float(ms[1]), int(nbytes[1]))}

    # ---- unhashed TF-IDF search (csrc/nearest.hip) -------------------------------------------------
    def set_weights(self, w):
        """The weight of every line (line_weights / load_weights): len(w) must be the store's line count, every weight
        0 or a finite number in [2^-200, 2^64]; ValueError otherwise.  No GPU work before the first search."""
        w = np.ascontiguousarray(w, np.float64)
        if w.ndim != 1:
            raise ValueError("set_weights takes one weight per line (a 1-d array)")
        check(lib().morna_jstore_set_weights(self._p, ptr(w), len(w)))

    def _nearest_out(self, nq, k):
        return np.zeros((nq, k), np.int32), np.zeros((nq, k), np.float64), np.zeros(nq, np.int32)

    def nearest(self, population, queries, k):
        """The k nearest samples of `population` (external sample ids; results are positions in it) to every query, a
        (lines ascending, coverages >= 0) pair each, by the unhashed cosine distance.  Returns (ids [nq][k] int32,
        distances [nq][k] fp64, counts [nq]): ascending distance, equal distances by descending position, -1 / +inf
        past min(k, len(population)).  IndexError for a population id the store lacks, ValueError for a negative
        coverage, unsorted lines, or k outside [1, 1024]."""
        pop = np.ascontiguousarray(population, np.int64)
        q_ptr, q_line, q_cov = _pack_queries(queries)
        ids, d, cnt = self._nearest_out(len(q_ptr) - 1, max(int(k), 1))
        check(lib().morna_jstore_nearest(self._p, ptr(pop), len(pop), ptr(q_ptr), ptr(q_line), ptr(q_cov), len(q_ptr) - 1, int(k),
                                         ptr(ids), ptr(d), ptr(cnt)))
        return ids, d, cnt

    def nearest_by_sample(self, population, query_sample_ids, k):
        """nearest() with the store's own rows as the queries (external sample ids, in the population or not): only ids
        go to the device."""
        pop = np.ascontiguousarray(population, np.int64)
        q = np.ascontiguousarray(query_sample_ids, np.int64)
        ids, d, cnt = self._nearest_out(len(q), max(int(k), 1))
        check(lib().morna_jstore_nearest_by_sample(self._p, ptr(pop), len(pop), ptr(q), len(q), int(k), ptr(ids), ptr(d), ptr(cnt)))
        return ids, d, cnt

    def nearest_stats(self):
        """Of the last nearest / nearest_by_sample: candidates re-ranked in all and the most for one query, passes over
        the store, kernel ms (HIP events), algorithmic bytes (8 per store entry of the population per pass), queries per
        pass, kernel ms of the row-norm pass (0.0 when the norms were cached), and the selection window."""
        return read_stats(lib().morna_jstore_nearest_stats, self._p, NEAREST_STATS)

    # ---- the junctions behind a query and each result (csrc/explain.hip) ---------------------------
    def _explained(self, r, n_res, top):
        """The Explained objects of a morna_jexplained, list by list; frees it."""
        try:
            out = []
            sums, counts, n_top = np.zeros(6, np.float64), np.zeros(3, np.int64), C.c_int32()
            pair = lib().morna_jexplained_pair
            p_sums, p_counts, p_top = ptr(sums), ptr(counts), C.byref(n_top)
            for q, n in enumerate(n_res.tolist()):
                pairs = []
                if n:                                          # a query's lists are [k][top], rank-major: one view of each
                    p = [C.c_void_p() for _ in range(3)]
                    check(pair(r, q, 0, None, None, None, *[C.byref(x) for x in p]))
                    lines, terms, cov_r = [view(x, t, n * top).reshape(n, top) for x, t in zip(p, (C.c_int32, C.c_double, C.c_int32))]
                for rank in range(n):
                    check(pair(r, q, rank, p_sums, p_counts, p_top, None, None, None))
                    m = n_top.value
                    pairs.append(Explained(sums.copy(), counts.copy(), lines[rank, :m], terms[rank, :m], cov_r[rank, :m]))
                out.append(pairs)
            return out
        finally:
            lib().morna_jexplained_free(r)

    def explain(self, queries, result_sample_ids, top):
        """For every query -- a (lines ascending, coverages >= 0) pair as nearest() takes them -- and every sample of its
        list in `result_sample_ids` (external ids in rank order, at most 1024 per list; an id may stand at several ranks),
        the decomposition of the unhashed cosine of the pair: one list of Explained per query.  All pairs in one call on
        the GPU.  IndexError for an id the store lacks, ValueError for a negative coverage, unsorted lines, or `top`
        outside [1, 64], RuntimeError without weights."""
        q_ptr, q_line, q_cov = _pack_queries(queries)
        nq = len(q_ptr) - 1
        res, n_res, k = _pack_lists(result_sample_ids, "explain takes at most %d", MAX_NEAREST)
        if len(n_res) != nq:
            raise ValueError("explain takes one result list per query (%d queries, %d lists)" % (nq, len(n_res)))
        r = C.c_void_p()
        check(lib().morna_jstore_explain(self._p, ptr(q_ptr), ptr(q_line), ptr(q_cov), nq, ptr(res), ptr(n_res), k, int(top),
                                         C.byref(r)))
        return self._explained(r, n_res, int(top))

    def explain_by_sample(self, query_sample_ids, result_sample_ids, top):
        """explain() with the store's own rows as the queries (external sample ids): only ids go to the device."""
        q = np.ascontiguousarray([int(s) for s in query_sample_ids], np.int64)
        res, n_res, k = _pack_lists(result_sample_ids, "explain takes at most %d", MAX_NEAREST)
        if len(n_res) != len(q):
            raise ValueError("explain takes one result list per query (%d queries, %d lists)" % (len(q), len(n_res)))
        r = C.c_void_p()
        check(lib().morna_jstore_explain_by_sample(self._p, ptr(q), len(q), ptr(res), ptr(n_res), k, int(top), C.byref(r)))
        return self._explained(r, n_res, int(top))

    def explain_stats(self):
        """Of the last explain / explain_by_sample: pairs explained, store entries streamed, passes (query tiles), kernel ms
        (HIP events), algorithmic bytes (8 per entry streamed) and queries per pass; all 0 after a refused call."""
        return read_stats(lib().morna_jstore_explain_stats, self._p, EXPLAIN_STATS)

    # ---- recovery tables over the filter grid -------------------------------------------------------
    def _recovery_arguments(self, result_sample_ids, coverage_grid, prefixes=None):
        """prefixes: of a sweep, which adds them (int32) to what is returned and an axis of their number to hist."""
        res, n_res, k = _pack_lists(result_sample_ids, "the recovery tables take at most %d, as the junction filter does")
        grid = np.array([_clamp62(c) for c in coverage_grid], np.int64)
        planes = (2, MAX_RESULTS + 1, max(min(len(grid), MAX_GRID), 0) + 1)
        if prefixes is None:
            return res, n_res, k, grid, np.zeros((len(n_res),) + planes, np.int32)
        pre = np.array([min(max(int(p), -2**31), 2**31 - 1) for p in prefixes], np.int32)
        return res, n_res, k, grid, pre, np.zeros((len(n_res), max(min(len(pre), MAX_PREFIXES), 1)) + planes, np.int32)

    def _truth_csr(self, truth_lines, n_lists):
        """truth_lines[q], line numbers, as (t_ptr int64 [nq + 1], t_line int32); ValueError for a line the store lacks."""
        truth = [np.ascontiguousarray(t, np.int64).reshape(-1) for t in truth_lines]
        if len(truth) != n_lists:
            raise ValueError("recovery takes one truth per result list (%d lists, %d truths)" % (n_lists, len(truth)))
        for q, t in enumerate(truth):
            if len(t) and (t.min() < 0 or t.max() >= self.n_lines):
                raise ValueError("the truth of list %d names line %d: the store has lines 0 to %d"
                                 % (q, int(t.min() if t.min() < 0 else t.max()), self.n_lines - 1))
        t_ptr = np.zeros(len(truth) + 1, np.int64)
        np.cumsum([len(t) for t in truth], out=t_ptr[1:])
        return t_ptr, np.concatenate(truth + [np.zeros(0, np.int64)]).astype(np.int32)

    def _truth_ids(self, truth_sample_ids, n_lists):
        truth = np.ascontiguousarray([int(t) for t in truth_sample_ids], np.int64)
        if len(truth) != n_lists:
            raise ValueError("recovery takes one truth per result list (%d lists, %d truths)" % (n_lists, len(truth)))
        return truth

    def recovery(self, result_sample_ids, truth_lines, coverage_grid):
        """For every list of `result_sample_ids` (external sample ids in rank order, at most 64 per list) and its truth --
        truth_lines[q]: line numbers, ascending and distinct -- the histogram from which every cell of a filter grid
        follows (recovery_rows): int64 [nq][2][65][B + 1], entry [q][t][cnt][b] the number of lines with truth bit t that
        cnt of the results hold and whose largest coverage among them reaches b of the B thresholds of `coverage_grid`
        (strictly ascending, at most 15); plane t = 0 is left 0 at cnt = 0.  One pass on the GPU; only the histogram
        comes back."""
        res, n_res, k, grid, hist = self._recovery_arguments(result_sample_ids, coverage_grid)
        t_ptr, t_line = self._truth_csr(truth_lines, len(n_res))
        check(lib().morna_jstore_recovery(self._p, ptr(res), ptr(n_res), len(n_res), k, ptr(t_ptr), ptr(t_line), ptr(grid),
                                          len(grid), ptr(hist)))
        return hist.astype(np.int64)

    def recovery_by_sample(self, result_sample_ids, truth_sample_ids, coverage_grid, truth_min_coverage=1):
        """recovery() with the truth of list q taken from the store's own row of truth_sample_ids[q] (an external id): its
        lines covered at least truth_min_coverage times.  Only ids go to the device."""
        res, n_res, k, grid, hist = self._recovery_arguments(result_sample_ids, coverage_grid)
        truth = self._truth_ids(truth_sample_ids, len(n_res))
        check(lib().morna_jstore_recovery_by_sample(self._p, ptr(res), ptr(n_res), len(n_res), k, ptr(truth),
                                                    _clamp62(truth_min_coverage), ptr(grid), len(grid), ptr(hist)))
        return hist.astype(np.int64)

    def recovery_sweep(self, result_sample_ids, truth_lines, coverage_grid, prefixes):
        """recovery() for several lengths of every list from one pass over its rows.  prefixes: list
        lengths, strictly ascending, each 1 to 64, at most 8.  Returns int64 [nq][P][2][65][B + 1]: [q][i] is what recovery()
        returns for list q cut to its first min(prefixes[i], len(list)) results, so its table is recovery_rows(hist[q][i],
        min(prefixes[i], len(list)), ...); results at or beyond the last prefix are not used."""
        res, n_res, k, grid, pre, hist = self._recovery_arguments(result_sample_ids, coverage_grid, prefixes)
        t_ptr, t_line = self._truth_csr(truth_lines, len(n_res))
        check(lib().morna_jstore_recovery_sweep(self._p, ptr(res), ptr(n_res), len(n_res), k, ptr(t_ptr), ptr(t_line), ptr(grid),
                                                len(grid), ptr(pre), len(pre), ptr(hist)))
        return hist.astype(np.int64)

    def recovery_sweep_by_sample(self, result_sample_ids, truth_sample_ids, coverage_grid, prefixes, truth_min_coverage=1):
        """recovery_sweep() with the truth of recovery_by_sample(): the store's own row of truth_sample_ids[q]."""
        res, n_res, k, grid, pre, hist = self._recovery_arguments(result_sample_ids, coverage_grid, prefixes)
        truth = self._truth_ids(truth_sample_ids, len(n_res))
        check(lib().morna_jstore_recovery_sweep_by_sample(self._p, ptr(res), ptr(n_res), len(n_res), k, ptr(truth),
                                                          _clamp62(truth_min_coverage), ptr(grid), len(grid), ptr(pre), len(pre),
                                                          ptr(hist)))
        return hist.astype(np.int64)

    def recovery_stats(self):
        """Of the last recovery / recovery_by_sample or sweep: kernel ms (HIP events), algorithmic bytes (8 per entry of the
        result and truth rows named, 4 per line of a truth given as lines; a sweep reads the rows up to its last prefix,
        once) and workgroups launched."""
        return read_stats(lib().morna_jstore_recovery_stats, self._p, RECOVERY_STATS)

    # ---- pooled samples -------------------------------------------------------------------------------
    def pool(self, groups):
        """One Pooled per group of `groups` (external sample ids, any number per group): every line at least one sample of
        the group holds, with the group's summed coverage and the number of its samples that hold it.  All groups in one
        call on the GPU.  An id repeated inside a group counts once, the first time (the `sample in wanted_ids` of
        create_supersample.py); IndexError for an id the store lacks."""
        groups = [list(dict.fromkeys(int(s) for s in grp)) for grp in groups]
        g_ptr = np.zeros(len(groups) + 1, np.int64)
        np.cumsum([len(grp) for grp in groups], out=g_ptr[1:])
        members = np.array([s for grp in groups for s in grp], np.int64)
        r = C.c_void_p()
        check(lib().morna_jstore_pool(self._p, ptr(members), ptr(g_ptr), len(groups), C.byref(r)))
        try:
            counts = np.zeros(len(groups), np.int64)
            check(lib().morna_jpooled_counts(r, ptr(counts)))
            out = []
            for g in range(len(groups)):
                p = [C.c_void_p() for _ in range(3)]
                check(lib().morna_jpooled_group(r, g, *[C.byref(x) for x in p]))
                n = int(counts[g])
                out.append(Pooled(view(p[0], C.c_int32, n), view(p[1], C.c_int64, n), view(p[2], C.c_int32, n)))
            return out
        finally:
            lib().morna_jpooled_free(r)

    def pool_stats(self):
        """Of the last pool: kernel ms (HIP events, both passes), bytes read (8 per entry of every member row, per pass),
        bytes written (16 per held line) and workgroups per pass."""
        return read_stats(lib().morna_jstore_pool_stats, self._p, POOL_STATS)

    # ---- depth thinning -----------------------------------------------------------------------------------
    def thin(self, sample_ids, keep, seed):
        """One Thinned per job (sample_ids[q], keep[q]): the row of that external sample id with every read kept when its
        hash is below keep[q], an integer in [0, 2^32] (parse_downsample: round(rate * 2^32)); a scalar `keep` serves every
        job.  The same id may be named by many jobs.  All jobs in one call on the GPU; the answer depends on (seed, sample
        id, line, coverage, keep) alone.  IndexError for an id the store lacks, ValueError for a threshold outside [0, 2^32]
        or a row with a coverage outside [0, 2^24]."""
        ids = np.ascontiguousarray([int(s) for s in sample_ids], np.int64)
        keep = [int(keep)] * len(ids) if np.ndim(keep) == 0 else [int(a) for a in keep]
        if len(keep) != len(ids):
            raise ValueError("thin takes one threshold per job (%d jobs, %d thresholds)" % (len(ids), len(keep)))
        for a in keep:
            if a < 0 or a > KEEP_ALL:
                raise ValueError("thin: the threshold %d is outside [0, 2^32]" % a)
        keep = np.array(keep, np.uint64)
        r = C.c_void_p()
        check(lib().morna_jstore_thin(self._p, ptr(ids), ptr(keep), len(ids), int(seed) & 0xffffffff, C.byref(r)))
        try:
            counts = np.zeros(len(ids), np.int64)
            check(lib().morna_jthinned_counts(r, ptr(counts)))
            out = []
            for q in range(len(ids)):
                p = [C.c_void_p() for _ in range(2)]
                check(lib().morna_jthinned_job(r, q, *[C.byref(x) for x in p]))
                n = int(counts[q])
                out.append(Thinned(view(p[0], C.c_int32, n), view(p[1], C.c_int32, n)))
            return out
        finally:
            lib().morna_jthinned_free(r)

    def thin_stats(self):
        """Of the last thin: kernel ms (HIP events: both passes and the scan), bytes read (16 per entry of every named row),
        bytes written (4 per entry and 8 per surviving line), draws made (the summed coverage of the named rows) and
        workgroups per pass."""
        return read_stats(lib().morna_jstore_thin_stats, self._p, THIN_STATS)

    # ---- hashed rows of any width (AnnoyIndex.add_items_from_store) ----------------------------------------
    def hash_rows_stats(self):
        """Of the last AnnoyIndex.add_items_from_store over this store: kernel ms (HIP events), bytes read (8 per entry of
        every named row, 12 per line for hash and weight), bytes written (4 per padded cell) and workgroups; all 0 after a
        refused call."""
        return read_stats(lib().morna_jstore_hash_rows_stats, self._p, HASH_ROWS_STATS)

    def row_norms(self, sample_ids):
        """The unhashed squared norm (fp64) of the store rows of `sample_ids` (external ids; repeats allowed) under the
        weights set: the pp of the unhashed search.  IndexError for an id the store lacks, RuntimeError without weights,
        ValueError for a row with a negative coverage."""
        ids = np.ascontiguousarray([int(s) for s in sample_ids], np.int64)
        out = np.zeros(len(ids), np.float64)
        check(lib().morna_jstore_row_norms(self._p, ptr(ids), len(ids), ptr(out)))
        return out

    def retain(self, result_sample_ids, frequency_filter, coverage_filter):
        """The retention step (morna.py:1539-1569) for every list of `result_sample_ids` (external sample ids in rank
        order, at most 64 per list) in one call on the GPU.  Returns one Retained per list."""
        res, n_res, k = _pack_lists(result_sample_ids, "the junction filter takes at most %d (found_in is one 64-bit word per line)")
        nq = len(n_res)
        minc = np.array([min(max(min_count(frequency_filter, int(n)), -1), MAX_RESULTS + 1) for n in n_res], np.int32)
        r = C.c_void_p()
        check(lib().morna_jstore_retain(self._p, ptr(res), ptr(n_res), ptr(minc), nq, k, _clamp62(coverage_filter), C.byref(r)))
        try:
            counts = np.zeros(nq, np.int64)
            check(lib().morna_jretained_counts(r, ptr(counts)))
            out = []
            for q in range(nq):
                n = int(counts[q])
                p = [C.c_void_p() for _ in range(4)]
                check(lib().morna_jretained_query(r, q, *[C.byref(x) for x in p]))
                cov_ptr = view(p[2], C.c_int64, n + 1)
                lo, hi = int(cov_ptr[0]), int(cov_ptr[-1])     # (an empty list: one offset, its place in the flat array)
                cov = view(C.c_void_p(p[3].value + 4 * lo) if p[3].value else p[3], C.c_int32, hi - lo)
                out.append(Retained(view(p[0], C.c_int32, n), view(p[1], C.c_uint64, n), cov_ptr - lo, cov))
            return out
        finally:
            lib().morna_jretained_free(r)


def line_weights(parsed, sample_threshold):
    """The unhashed search's weight of every line of a threshold-0 parse: the parse's own idf,
    log(float(sample_count) / samples listed) (morna.py:372-374), for a line that lists at least `sample_threshold`
    samples, 0.0 for a line the index skipped.  None when a "chrom start end" key repeats in the file: the index then
    weighs a line by its key's cumulative frequency and sums the repeats into one term, which is not this definition."""
    if parsed.n_keys != parsed.lines_read or parsed.n_lines != parsed.lines_read:
        return None
    a = parsed.arrays()
    w = np.array(a["idf"], np.float64)
    w[np.diff(a["row_ptr"]) < int(sample_threshold)] = 0.0
    return w


def save_weights(path, w, sample_count, sample_threshold):
    """<basename>.jw.mor: "MORNAJW1", n_lines, sample_count, threshold (int64 each), w[n_lines] fp64, little-endian."""
    import os
    w = np.ascontiguousarray(w, "<f8")
    tmp = "%s.tmp.%d" % (path, os.getpid())
    with open(tmp, "wb") as fh:
        fh.write(WEIGHTS_MAGIC)
        fh.write(np.array([len(w), int(sample_count), int(sample_threshold)], "<i8").tobytes())
        fh.write(w.tobytes())
    os.replace(tmp, path)


def load_weights(path, n_lines=None):
    """(w, sample_count, sample_threshold) of a weights file; IOError for a missing or truncated file, one that is not a
    weights file, or one whose line count is not `n_lines` (the store's)."""
    try:
        with open(path, "rb") as fh:
            blob = fh.read()
    except (IOError, OSError) as e:
        raise IOError("%s: %s" % (path, e))
    if len(blob) < 32 or blob[:8] != WEIGHTS_MAGIC:
        raise IOError("%s is not a weights file of the unhashed search (or is truncated)" % path)
    n, sample_count, threshold = [int(x) for x in np.frombuffer(blob, "<i8", 3, 8)]
    if n < 0 or len(blob) != 32 + 8 * n:
        raise IOError("%s is truncated or damaged: %d bytes do not hold %d weights" % (path, len(blob), n))
    if n_lines is not None and n != int(n_lines):
        raise IOError("%s holds the weights of %d lines, the junction store has %d: they are not of the same index"
                      % (path, n, int(n_lines)))
    return np.frombuffer(blob, "<f8", n, 32).astype(np.float64), sample_count, threshold


def build_store(intropolis, basename, sample_count, device=0, sample_threshold=None):
    """`morna index --junction-store`: the intropolis file parsed once more with threshold 0 -- every line kept, so kept
    line j is file line j -- then transposed on the GPU and saved as <basename>.junc.mor.  With the index's
    sample_threshold, the same parse also gives <basename>.jw.mor, the line weights of `search --unhashed` -- unless a key
    repeats in the file (line_weights), which one line on stderr reports."""
    from .index import ParsedLines
    parsed = ParsedLines(intropolis, sample_count=max(1, int(sample_count or 0)), sample_threshold=0)
    store = JunctionStore.build(parsed, device=device)
    store.save(basename + STORE_SUFFIX)
    write_weights(parsed, basename, sample_threshold, intropolis)
    return store


def write_weights(parsed, basename, sample_threshold, source="the indexed file"):
    """<basename>.jw.mor from the threshold-0 parse of the indexed file; True when written.  A weights file of an earlier
    index goes first; sample_threshold None writes none; a file with repeated junctions gets none and one line on stderr."""
    import os
    import sys
    path = basename + WEIGHTS_SUFFIX
    if os.path.exists(path):
        os.remove(path)
    if sample_threshold is None:
        return False
    w = line_weights(parsed, sample_threshold)
    if w is None:
        sys.stderr.write("%s not written: the %d lines of %s hold %d distinct junctions, and the unhashed search is defined "
                         "for files without repeated junctions\n" % (path, parsed.lines_read, source, parsed.n_keys))
        return False
    save_weights(path, w, parsed.sample_count, sample_threshold)
    return True


def remove_stale_store(basename):
    """An index written without --junction-store must not be found next to the store of an earlier one, nor next to
    that store's weights."""
    import os
    for suffix in (STORE_SUFFIX, WEIGHTS_SUFFIX):
        if os.path.exists(basename + suffix):
            os.remove(basename + suffix)


def _line_keys(parsed):
    """The "chrom start end" key of every line of a parse, in line order."""
    a = parsed.arrays()
    blob, off = a["key_bytes"].tobytes(), a["key_off"].tolist()
    return [blob[off[j]:off[j + 1]].decode("ascii") for j in range(parsed.n_lines)]


def _sum_cells(sample, code, cov, span):
    """(sample, code, summed coverage) of every distinct (sample, code) cell, code in [0, span), ascending."""
    cell, inv = np.unique(np.asarray(sample, np.int64) * span + code, return_inverse=True)
    total = np.zeros(len(cell), np.int64)
    np.add.at(total, inv.reshape(-1), np.asarray(cov, np.int64))
    return cell // span, cell % span, total


def key_lines(junction_file, n_lines=None):
    """"chrom start end" -> line number of the indexed intropolis file, from the key arrays of a threshold-0 parse;
    ValueError when the file's line count is not `n_lines` (the store's)."""
    from .index import ParsedLines
    parsed = ParsedLines(junction_file, sample_count=1, sample_threshold=0)
    if n_lines is not None and parsed.lines_read != int(n_lines):
        raise ValueError("%s has %d lines, the junction store has %d: it is not the file that was indexed"
                         % (junction_file, parsed.lines_read, int(n_lines)))
    return {key: j for j, key in enumerate(_line_keys(parsed))}


def line_hashes(junction_file, n_lines, handle):
    """The int32 hash of every line's "chrom start end" key (mmh3.hash, morna.py:369), in line order, from the key arrays
    of a threshold-0 parse of the indexed file through morna_hash_keys on `handle` (an AnnoyIndex; its items are not
    touched): what AnnoyIndex.add_items_from_store takes.  ValueError when the file's line count is not `n_lines` (the
    store's)."""
    from .index import ParsedLines
    parsed = ParsedLines(junction_file, sample_count=1, sample_threshold=0)
    if n_lines is not None and parsed.lines_read != int(n_lines):
        raise ValueError("%s has %d lines, the junction store has %d: it is not the file that was indexed"
                         % (junction_file, parsed.lines_read, int(n_lines)))
    a = parsed.arrays()
    return handle.hash_keys(a["key_bytes"], a["key_off"])[0]


def query_terms(coverage_by_key, key_line, w):
    """One unhashed query: {"chrom start end": summed coverage} -> (lines ascending, coverages) int32 arrays.  Keys the
    file lacks and keys on lines of weight 0 drop out."""
    pairs = sorted((key_line[key], int(c)) for key, c in coverage_by_key.items() if key in key_line and w[key_line[key]] != 0.0)
    return (np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32))


def intropolis_query_terms(path, key_line, w):
    """Every sample of the intropolis file `path` as an unhashed query: (sample ids in first-seen order, one
    (lines, coverages) pair per sample), the coverages of a key the file repeats summed per sample as update_query and
    morna_lines_query_terms sum them."""
    from .index import ParsedLines
    parsed = ParsedLines(path, sample_count=1, sample_threshold=0)
    a = parsed.arrays()
    at = np.array([key_line.get(key, -1) for key in _line_keys(parsed)], np.int64)
    at[at >= 0] = np.where(np.asarray(w)[at[at >= 0]] != 0.0, at[at >= 0], -1)
    line = np.repeat(at, np.diff(a["row_ptr"]))
    keep = line >= 0
    sample, line, cov = _sum_cells(a["ids"][keep], line[keep], a["cov"][keep], max(len(w), 1))
    if len(cov) and cov.max() > 2**31 - 1:
        raise ValueError("%s: a query sample's summed coverage of one junction passes 2^31 - 1" % path)
    cut = np.searchsorted(sample, np.arange(parsed.n_items + 1))
    terms = [(line[cut[s]:cut[s + 1]].astype(np.int32), cov[cut[s]:cut[s + 1]].astype(np.int32)) for s in range(parsed.n_items)]
    return [int(x) for x in a["ext_ids"]], terms


def intropolis_truth(path, key_line, min_coverage=1):
    """The truth sets of `morna recovery --truth`: for every sample of the intropolis file `path`, {sample id: (lines,
    extra)} -- the ascending line numbers (through key_line, key_lines of the indexed file) of the junctions it covers
    at least min_coverage times, the coverages of a key the file repeats summed, and the number of such junctions that
    are no line of the indexed file."""
    from .index import ParsedLines
    parsed = ParsedLines(path, sample_count=1, sample_threshold=0)
    a = parsed.arrays()
    unknown = {}
    at = np.array([key_line[key] if key in key_line else -1 - unknown.setdefault(key, len(unknown))
                   for key in _line_keys(parsed)], np.int64)
    span = max(len(key_line), int(at.max()) + 1 if len(at) else 0, 1) + len(unknown)
    code = np.repeat(at + len(unknown), np.diff(a["row_ptr"]))           # unknown keys first, then the lines
    sample, code, cov = _sum_cells(a["ids"], code, a["cov"], span)
    sample, code = sample[cov >= int(min_coverage)], code[cov >= int(min_coverage)] - len(unknown)
    cut = np.searchsorted(sample, np.arange(parsed.n_items + 1))
    out = {}
    for s, ext in enumerate(a["ext_ids"].tolist()):
        mine = code[cut[s]:cut[s + 1]]
        out[int(ext)] = (mine[mine >= 0].astype(np.int32), int((mine < 0).sum()))
    return out


def _open_text(path):
    with open(path, "rb") as fh:
        gz = fh.read(2) == b"\x1f\x8b"
    return gzip.open(path, "rt") if gz else open(path, "r")


def write_splice_files(junction_file, jobs):
    """The output loop of morna.py:1582-1635 for several queries in one pass over `junction_file`.

    jobs: (path, Retained, result_sample_ids) per query.  For every retained line j, ascending, line j of the file is
    written with tokens[1] - 2, the sample ids of found_in[j] in rank order, their coverages, and str(found_in[j]) as
    one more field.  The named samples must be in the line's own sample list with the same coverage (the reference's
    old_samples.index look-up, here the check that the file is the one indexed): ValueError naming the line otherwise.
    An empty retained set writes an empty file."""
    jobs = list(jobs)
    handles = [open(path, "w") for path, _, _ in jobs]
    try:
        if not jobs:
            return
        # every (line, job, position in the job's list), by line
        line = np.concatenate([np.asarray(r.lines, np.int64) for _, r, _ in jobs])
        job = np.concatenate([np.full(len(r.lines), i, np.int64) for i, (_, r, _) in enumerate(jobs)])
        pos = np.concatenate([np.arange(len(r.lines), dtype=np.int64) for _, r, _ in jobs])
        order = np.lexsort((job, line))
        line, job, pos = line[order].tolist(), job[order].tolist(), pos[order].tolist()
        if not line:
            return
        found = [r.found_in for _, r, _ in jobs]
        covs = [r.coverages for _, r, _ in jobs]
        at = 0
        with _open_text(junction_file) as names:
            for i, text in enumerate(names):
                if line[at] != i:
                    continue
                tokens = text.strip().split("\t")
                if len(tokens) < 8:
                    raise ValueError("line %d of %s has %d tab-separated fields, an intropolis line has 8" % (i, junction_file, len(tokens)))
                start = str(int(tokens[1]) - 2)
                old = dict(zip((int(x) for x in tokens[6].split(",")), (int(x) for x in tokens[7].split(","))))
                while at < len(line) and line[at] == i:
                    q, p = job[at], pos[at]
                    ranks = found[q][p]
                    sample_ids = [jobs[q][2][r] for r in ranks]
                    cov = covs[q][p]
                    for s, c in zip(sample_ids, cov):
                        if old.get(s) != c:
                            raise ValueError("line %d of %s does not list sample %d with coverage %d: it is not the file "
                                             "that was indexed" % (i, junction_file, s, c))
                    out = list(tokens)
                    out[1] = start
                    out[6] = ",".join(str(s) for s in sample_ids)
                    out[7] = ",".join(str(c) for c in cov)
                    handles[q].write("\t".join(out) + "\t" + str(ranks) + "\n")
                    at += 1
                if at == len(line):
                    break
        if at < len(line):
            raise ValueError("%s ends before line %d: it is not the file that was indexed" % (junction_file, line[at]))
    finally:
        for fh in handles:
            fh.close()


# ---- the junctions behind a result: the lines of `morna explain` ---------------------------------------
def line_names(junction_file, lines):
    """{line number: "chrom start end"} for the line numbers `lines` of `junction_file`, from one pass over the file that
    keeps only the lines asked for and stops behind the last.  ValueError when the file ends before one of them or a
    line has fewer than three fields."""
    wanted = sorted(set(int(j) for j in lines))
    names = {}
    if not wanted:
        return names
    at = 0
    with _open_text(junction_file) as fh:
        for i, text in enumerate(fh):
            if i != wanted[at]:
                continue
            pieces = text.split()
            if len(pieces) < 3:
                raise ValueError("line %d of %s has %d fields, a junction has at least 3" % (i, junction_file, len(pieces)))
            names[i] = " ".join(pieces[:3])
            at += 1
            if at == len(wanted):
                break
    if at < len(wanted):
        raise ValueError("%s ends before line %d: it is not the file that was indexed" % (junction_file, wanted[at]))
    return names


def explain_rows(pair, q_lines, q_cov, w, names=None):
    """What `morna explain` prints for one Explained: (summary, rows).  summary: (unhashed distance, shared, the share of the
    query's squared weight outside the intersection, the share of the result's, the share of pq the top list carries);
    rows, one per top entry: ("chrom start end" from `names`, or the line number without them; the query's coverage,
    looked up in its row (q_lines ascending, q_cov); the result's coverage; the line's weight; its share of pq).  A
    share whose denominator is 0 is nan.  Pure host code."""
    q_lines, q_cov = np.asarray(q_lines, np.int64), np.asarray(q_cov, np.int64)
    terms = [float(t) for t in pair.terms]
    pq = float(pair.pq)
    share = lambda x: x / pq if pq > 0 else float("nan")
    rows = []
    for l, t, c in zip([int(x) for x in pair.lines], terms, [int(x) for x in pair.cov_r]):
        at = int(np.searchsorted(q_lines, l))
        if at >= len(q_lines) or q_lines[at] != l:
            raise ValueError("line %d of a top list is not in the query's row: the row is not the one that was explained" % l)
        rows.append((names[l] if names is not None else l, int(q_cov[at]), c, float(w[l]), share(t)))
    return (float(pair.distance), int(pair.shared), pair.query_outside, pair.result_outside, share(sum(terms))), rows


def _explain_cell(v):
    if isinstance(v, float):
        return "nan" if v != v else "%.6f" % v
    return str(v)


def format_explain_rows(rank, shown_id, sample_id, search_distance, summary, rows=(), meta=None):
    """One pair of `morna explain`: the line "rank. id sample-id search-distance distance shared query-outside
    result-outside top-share" (tab-separated; `id` as `search` prints it, both distances as `search -d` prints them, the
    shares as %.6f or nan; `meta` appended as `search -m` appends it), then one line per row of explain_rows, led by a tab:
    junction, query coverage, result coverage, weight (as str of the float), share of pq."""
    dist = lambda d: "nan" if d != d else str(float(d))
    head = [str(rank) + ".", str(shown_id), str(sample_id), dist(search_distance), dist(summary[0]), str(summary[1])]
    head += [_explain_cell(float(x)) for x in summary[2:]]
    if meta is not None:
        head.append(str(meta))
    out = ["\t".join(head) + "\n"]
    for name, cov_q, cov_r, weight, share in rows:
        out.append("\t%s\t%d\t%d\t%s\t%s\n" % (name, cov_q, cov_r, str(float(weight)), _explain_cell(float(share))))
    return "".join(out)


# ---- pooled samples: the files of create_supersample.py ----------------------------------------------
_LABEL = re.compile(r"[A-Za-z0-9._-]+\Z")


def parse_sample_ids_file(path):
    """The --sampleids file of create_supersample.py: one integer sample id per line; blank lines are ignored.  ValueError
    naming the line otherwise."""
    ids = []
    with open(path) as fh:
        for n, text in enumerate(fh, 1):
            if not text.strip():
                continue
            try:
                ids.append(int(text))
            except ValueError:
                raise ValueError("line %d of %s is not an integer sample id (got %r)" % (n, path, text.strip()))
    return ids


def parse_groups_file(path):
    """A groups file, "<label><TAB><id>,<id>,..." per line, as [(label, [ids])] in file order.  Labels match
    [A-Za-z0-9._-]+ and are distinct; a label alone, or followed by a tab and nothing, is an empty group; blank lines are
    ignored.  ValueError naming the line otherwise."""
    groups, seen = [], set()
    with open(path) as fh:
        for n, text in enumerate(fh, 1):
            text = text.rstrip("\r\n")
            if not text.strip():
                continue
            parts = text.split("\t")
            if len(parts) > 2:
                raise ValueError("line %d of %s has %d tab-separated fields: a group is <label><TAB><id>,<id>,..."
                                 % (n, path, len(parts)))
            label = parts[0]
            if not _LABEL.match(label):
                raise ValueError("line %d of %s: the label %r is not made of letters, digits, '.', '_' and '-'" % (n, path, label))
            if label in seen:
                raise ValueError("line %d of %s: the label %r names a second group" % (n, path, label))
            seen.add(label)
            ids = []
            if len(parts) == 2 and parts[1].strip():
                for t in parts[1].split(","):
                    try:
                        ids.append(int(t))
                    except ValueError:
                        raise ValueError("line %d of %s: %r is not an integer sample id" % (n, path, t.strip()))
            groups.append((label, ids))
    return groups


def write_supersample_files(junction_file, jobs):
    """The output loop of create_supersample.py for several groups in one pass over `junction_file`.

    jobs: (path, Pooled) per group.  For EVERY line of the file: its first three whitespace-separated fields joined by
    tabs, a tab, the group's summed coverage of the line -- 0 where none of its samples holds it -- and a newline.
    ValueError when the file ends before a pooled line or a line has fewer than three fields."""
    jobs = list(jobs)
    handles = [open(path, "w") for path, _ in jobs]
    try:
        if not jobs:
            return
        last = max([int(r.lines[-1]) for _, r in jobs if len(r)] + [-1])
        at = [0] * len(jobs)
        lines = [np.asarray(r.lines).tolist() for _, r in jobs]
        sums = [np.asarray(r.sums).tolist() for _, r in jobs]
        i = -1
        with _open_text(junction_file) as names:
            for i, text in enumerate(names):
                pieces = text.split()
                if len(pieces) < 3:
                    raise ValueError("line %d of %s has %d fields, a junction has at least 3" % (i, junction_file, len(pieces)))
                head = "\t".join(pieces[:3]) + "\t"
                for q, fh in enumerate(handles):
                    a = at[q]
                    if a < len(lines[q]) and lines[q][a] == i:
                        fh.write(head + str(sums[q][a]) + "\n")
                        at[q] = a + 1
                    else:
                        fh.write(head + "0\n")
        if i < last:
            raise ValueError("%s ends before line %d: it is not the file that was indexed" % (junction_file, last))
    finally:
        for fh in handles:
            fh.close()
