"""The unhashed TF-IDF search, host side: the weights file, the weights themselves, set_weights'
validation, the command line's refusals and the term building of queries from outside the index.  Also holds the
yardstick test_gpu_unhashed.py compares the GPU with: a restatement of the contract in numpy, one rounding per
operation, fed the text lines.  No GPU."""
import gzip
import os
from math import log

import numpy as np
import pytest

from test_junctions_cpu import store_arrays, tiny_lines


# ---- the restatement -----------------------------------------------------------------------------------------------------
def ref_weights(lines, sample_count, threshold):
    """w[j]: log(float(sample_count) / samples listed) for a line of at least `threshold` samples, else 0.0."""
    w = []
    for text in lines:
        n = len(text.strip().split("\t")[6].split(","))
        w.append(log(float(sample_count) / n) if n >= threshold else 0.0)
    return np.array(w, np.float64)


def ref_items(lines, threshold):
    """External sample ids in internal-id order: first seen over the lines the index keeps (morna.py:361-382)."""
    items = {}
    for text in lines:
        samples = text.strip().split("\t")[6].split(",")
        if len(samples) >= threshold:
            for s in samples:
                items.setdefault(int(s), len(items))
    return list(items)


def ref_rows(lines):
    """sample id -> (line numbers ascending, coverages), over ALL lines."""
    rows = {}
    for j, text in enumerate(lines):
        t = text.strip().split("\t")
        for s, c in zip(t[6].split(","), t[7].split(",")):
            rows.setdefault(int(s), ([], []))
            rows[int(s)][0].append(j)
            rows[int(s)][1].append(int(c))
    return rows


class RefUnhashed(object):
    """The contract over a population of (lines, coverages) rows.  A sequential sum is np.cumsum along a row of terms
    (one rounding per addition, in order); a row shorter than the longest is padded with terms +0.0, which change no
    sum of non-negative terms."""

    def __init__(self, pop_rows, w):
        self.w = np.asarray(w, np.float64)
        self.n = len(pop_rows)
        width = max([len(l) for l, _ in pop_rows] + [1])
        self.line = np.zeros((self.n, width), np.int64)
        self.v = np.zeros((self.n, width), np.float64)
        for i, (l, c) in enumerate(pop_rows):
            self.line[i, :len(l)] = l
            self.v[i, :len(l)] = np.asarray(c, np.float64) * self.w[np.asarray(l, np.int64)]     # RN(double(cov) * w)
        self.pp = np.cumsum(self.v * self.v, axis=1)[:, -1]

    def radicands(self, q_lines, q_cov):
        q_lines = np.asarray(q_lines, np.int64)
        qv = np.asarray(q_cov, np.float64) * self.w[q_lines]
        qq = float(np.cumsum(np.concatenate([[0.0], qv * qv]))[-1])
        dense = np.zeros(len(self.w), np.float64)
        dense[q_lines] = qv
        pq = np.cumsum(self.v * dense[self.line], axis=1)[:, -1]
        ppqq = self.pp * qq
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(ppqq > 0, 2.0 - 2.0 * pq / np.sqrt(ppqq), 2.0)

    def distances(self, q_lines, q_cov):
        return np.sqrt(np.maximum(self.radicands(q_lines, q_cov), 0.0))

    def nearest(self, q_lines, q_cov, k):
        """(ids, distances): ascending distance, equal distances higher id first; at most the population."""
        d = self.distances(q_lines, q_cov)
        order = sorted(range(self.n), key=lambda i: (d[i], -i))[:k]
        return order, [float(d[i]) for i in order]


def ref_query_terms(coverage_by_key, lines, w):
    """key -> line from the text lines, then the terms of one query: (line, coverage) ascending, keys the file lacks and
    lines of weight 0 dropped."""
    key_line = {" ".join(text.split("\t")[:3]): j for j, text in enumerate(lines)}
    terms = {}
    for key, cov in coverage_by_key.items():
        j = key_line.get(key)
        if j is not None and w[j] != 0.0:
            terms[j] = terms.get(j, 0) + cov
    return sorted(terms.items())


# ---- weights and their file ----------------------------------------------------------------------------------------------
def _write_gz(path, lines):
    with gzip.open(path, "wt") as fh:
        fh.write("".join(lines))


def _parsed(tmp_path, lines, sample_count, name="f.gz"):
    from morna_amd.index import ParsedLines
    path = str(tmp_path / name)
    _write_gz(path, lines)
    return ParsedLines(path, sample_count=sample_count, sample_threshold=0)


@pytest.mark.parametrize("name,sample_count,threshold,zeros", [("generic", 10, 4, 18), ("generic", 10, 1, 1),
                                                                ("tiny", 21504, 100, 0), ("tiny", 30000, 2000, 1)])
def test_weights_are_the_parse_idf_or_zero(tmp_path, embedded, name, sample_count, threshold, zeros):
    from morna_amd.junctions import line_weights
    lines = embedded["generic"] if name == "generic" else tiny_lines()
    w = line_weights(_parsed(tmp_path, lines, sample_count), threshold)
    want = ref_weights(lines, sample_count, threshold)
    assert w.dtype == np.float64 and w.tobytes() == want.tobytes()
    assert (want == 0).sum() == zeros


def test_weights_file_round_trip_and_damage(tmp_path, embedded):
    from morna_amd.junctions import WEIGHTS_SUFFIX, load_weights, write_weights
    lines = embedded["generic"]
    base = str(tmp_path / "idx")
    assert write_weights(_parsed(tmp_path, lines, 10), base, 4) is True
    path = base + WEIGHTS_SUFFIX
    w, sample_count, threshold = load_weights(path, len(lines))
    assert (sample_count, threshold) == (10, 4)
    assert w.tobytes() == ref_weights(lines, 10, 4).tobytes()
    assert load_weights(path)[0].tobytes() == w.tobytes()
    with open(path, "rb") as fh:
        blob = fh.read()
    assert len(blob) == 32 + 8 * len(lines) and blob[:8] == b"MORNAJW1"
    with pytest.raises(IOError):
        load_weights(path, len(lines) + 1)                   # the store has another line count
    with pytest.raises(IOError):
        load_weights(str(tmp_path / "absent.jw.mor"))
    for name, damaged in (("short", blob[:-3]), ("long", blob + b"\0"), ("head", blob[:20]), ("magic", b"X" + blob[1:]),
                          ("empty", b"")):
        bad = str(tmp_path / name)
        with open(bad, "wb") as fh:
            fh.write(damaged)
        with pytest.raises(IOError):
            load_weights(bad)
    # a later index without weights (no threshold given) removes the file
    assert write_weights(_parsed(tmp_path, lines, 10), base, None) is False and not os.path.exists(path)


def test_repeated_key_file_gets_no_weights_and_unhashed_says_why(tmp_path, embedded, capsys):
    from morna_amd.junctions import STORE_SUFFIX, WEIGHTS_SUFFIX, JunctionStore, line_weights, write_weights
    from morna_amd.search import MornaSearch
    lines = list(embedded["generic"])
    first = lines[0].split("\t")
    lines.append("\t".join(first[:6] + ["7,8", "1,1"]) + "\n")          # line 0's junction once more
    parsed = _parsed(tmp_path, lines, 10)
    assert parsed.n_keys == len(lines) - 1 and line_weights(parsed, 4) is None
    base = str(tmp_path / "idx")
    with open(base + WEIGHTS_SUFFIX, "wb") as fh:                          # left by an earlier index of the basename
        fh.write(b"stale")
    assert write_weights(parsed, base, 4, "f.gz") is False
    err = capsys.readouterr().err
    assert not os.path.exists(base + WEIGHTS_SUFFIX)
    assert err.count("\n") == 1 and "repeated junctions" in err and base + WEIGHTS_SUFFIX in err
    # the search side: a store without weights
    ext, ptr, line, cov, n_lines = store_arrays(lines)
    JunctionStore.from_arrays(ext, ptr, line, cov, n_lines).save(base + STORE_SUFFIX)
    s = MornaSearch.__new__(MornaSearch)
    s.basename, s._junction_store, s.annoy_index, s._device = base, None, None, 0
    with pytest.raises(IOError) as e:
        s.unhashed_store()
    assert "repeat" in str(e.value) and "--junction-store" in str(e.value)


def test_stale_weights_are_removed_with_the_store(tmp_path):
    from morna_amd.junctions import STORE_SUFFIX, WEIGHTS_SUFFIX, remove_stale_store
    base = str(tmp_path / "idx")
    for suffix in (STORE_SUFFIX, WEIGHTS_SUFFIX):
        with open(base + suffix, "wb") as fh:
            fh.write(b"x")
    remove_stale_store(base)
    assert not os.path.exists(base + STORE_SUFFIX) and not os.path.exists(base + WEIGHTS_SUFFIX)
    remove_stale_store(base)


# ---- set_weights ---------------------------------------------------------------------------------------------------------
def test_set_weights_validation(embedded):
    from morna_amd.junctions import JunctionStore
    ext, ptr, line, cov, n_lines = store_arrays(embedded["generic"])
    store = JunctionStore.from_arrays(ext, ptr, line, cov, n_lines)
    good = ref_weights(embedded["generic"], 10, 4)
    store.set_weights(good)
    store.set_weights(np.zeros(n_lines))
    store.set_weights(np.full(n_lines, 2.0 ** 64))
    for j, bad in ((3, float("nan")), (0, -1.0), (19, float("inf")), (5, 2.0 ** 65), (7, -float("inf")), (2, 1e-300)):
        w = good.copy()
        w[j] = bad
        with pytest.raises(ValueError) as e:
            store.set_weights(w)
        assert "line %d " % j in str(e.value)
    for n in (n_lines - 1, n_lines + 1, 0):
        with pytest.raises(ValueError) as e:
            store.set_weights(np.ones(n))
        assert "%d lines" % n_lines in str(e.value)
    with pytest.raises(ValueError):
        store.set_weights(np.ones((n_lines, 1)))


def test_nearest_needs_weights_and_a_k_in_range(embedded):
    from morna_amd.junctions import MAX_NEAREST, JunctionStore
    ext, ptr, line, cov, n_lines = store_arrays(embedded["generic"])
    store = JunctionStore.from_arrays(ext, ptr, line, cov, n_lines)
    with pytest.raises(RuntimeError) as e:
        store.nearest_by_sample(ext, ext[:1], 3)
    assert "set_weights" in str(e.value)
    store.set_weights(ref_weights(embedded["generic"], 10, 4))
    assert MAX_NEAREST >= 255
    for k in (0, -1, MAX_NEAREST + 1):
        with pytest.raises(ValueError) as e:
            store.nearest_by_sample(ext, ext[:1], k)
        assert str(MAX_NEAREST) in str(e.value)
    ids, d, cnt = store.nearest_by_sample(ext, [], 3)                    # no query: no GPU work either
    assert ids.shape == (0, 3) and d.shape == (0, 3) and len(cnt) == 0
    ids, d, cnt = store.nearest_by_sample([], ext[:2], 3)               # an empty population
    assert (ids == -1).all() and np.isinf(d).all() and cnt.tolist() == [0, 0]
    with pytest.raises(IndexError) as e:
        store.nearest_by_sample([], [12345], 3)
    assert "12345" in str(e.value)
    for lines_, covs in (([3, 2], [1, 1]), ([2, 2], [1, 1]), ([n_lines], [1]), ([-1], [1]), ([1], [-5])):
        with pytest.raises(ValueError):
            store.nearest([], [(lines_, covs)], 3)


# ---- the command line ----------------------------------------------------------------------------------------------------
def test_unhashed_parser_flags():
    from morna_amd import cli
    p = cli.build_parser()
    a = p.parse_args(["search", "-x", "idx", "--unhashed", "-q", "3"])
    assert a.unhashed is True and a.unhashed_junction_file is None and a.search_k == 100
    a = p.parse_args(["search", "-x", "idx", "--unhashed", "--junction-file", "j.gz", "-f", "raw"])
    assert a.unhashed_junction_file == "j.gz"
    a = p.parse_args(["search", "-x", "idx", "--search-k", "7"])
    assert a.unhashed is False and a.search_k == 7


@pytest.mark.parametrize("argv", [
    ["search", "-x", "idx", "--unhashed", "-q", "3", "-e"],
    ["search", "-x", "idx", "--unhashed", "-q", "3", "--search-k", "50"],
    ["search", "-x", "idx", "--unhashed", "-q", "3", "--search-k", "100"],                      # the default, but named
    ["search", "-x", "idx", "--unhashed", "--junction-file", "j.gz", "-c", "10"],
    ["search", "-x", "idx", "--unhashed", "--junction-file", "j.gz", "-rl"],
    ["search", "-x", "idx", "--unhashed", "-f", "raw"],                                         # a stream, no --junction-file
    ["search", "-x", "idx", "--unhashed", "--intropolis", "q.gz"],
    ["search", "-x", "idx", "--unhashed", "--query-ids", "1,2", "-e"],
    ["junctions", "-x", "idx", "--junction-file", "j.gz", "-sf", "o", "--unhashed", "-q", "3"],
])
def test_unhashed_parser_errors(argv, capsys):
    from morna_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    assert "--unhashed" in capsys.readouterr().err


def test_unhashed_refuses_one_process_per_shard(tmp_path, monkeypatch):
    from morna_amd import cli
    base = str(tmp_path / "idx")
    with open(base + ".shards.mor", "w") as fh:
        fh.write("2\n0 5 10\n")
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(RuntimeError) as e:
        cli.main(["search", "-x", base, "--unhashed", "-q", "3"])
    assert "batch search is not available with one process per shard" in str(e.value)


# ---- terms of a query from outside the index -------------------------------------------------------------------------------
def test_key_lines_and_query_terms_equal_the_restatement(tmp_path, embedded):
    from morna_amd.junctions import intropolis_query_terms, key_lines, query_terms
    lines = embedded["generic"]
    src = str(tmp_path / "junctions.gz")
    _write_gz(src, lines)
    w = ref_weights(lines, 10, 2)
    assert (w != 0).sum() == 3 and w[16] == 0                  # (line 16 lists all 10 samples: log(10 / 10))
    key_line = key_lines(src, len(lines))
    assert key_line == {" ".join(t.split("\t")[:3]): j for j, t in enumerate(lines)}
    with pytest.raises(ValueError) as e:
        key_lines(src, len(lines) + 1)
    assert "not the file that was indexed" in str(e.value)
    heavy = [j for j in range(len(lines)) if w[j] != 0]
    keys = [" ".join(t.split("\t")[:3]) for t in lines]
    query = {keys[heavy[2]]: 5, keys[heavy[0]]: 2, keys[0]: 9, keys[16]: 3, "chrZ 1 2": 4}
    got = query_terms(query, key_line, w)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    assert list(zip(got[0].tolist(), got[1].tolist())) == ref_query_terms(query, lines, w) == [(heavy[0], 2), (heavy[2], 5)]
    empty = query_terms({"chrZ 1 2": 4}, key_line, w)
    assert len(empty[0]) == 0 and len(empty[1]) == 0
    # a query file: its samples in first-seen order, a junction it repeats summed per sample, unknown junctions dropped
    def qline(j, samples, covs):
        return "\t".join(lines[j].split("\t")[:6] + [",".join(map(str, samples)), ",".join(map(str, covs))]) + "\n"
    qfile = [qline(heavy[1], [70, 50], [3, 4]), "chrZ\t1\t2\t+\tGT\tAG\t50,60\t8,8\n", qline(heavy[0], [50], [1]),
             qline(heavy[1], [50, 90], [10, 2]), qline(16, [90], [6])]
    qpath = str(tmp_path / "queries.gz")
    _write_gz(qpath, qfile)
    sample_ids, terms = intropolis_query_terms(qpath, key_line, w)
    assert sample_ids == [70, 50, 60, 90]
    want = {}
    for text in qfile:
        t = text.strip().split("\t")
        for s, c in zip(t[6].split(","), t[7].split(",")):
            d = want.setdefault(int(s), {})
            d[" ".join(t[:3])] = d.get(" ".join(t[:3]), 0) + int(c)
    for s, (l, c) in zip(sample_ids, terms):
        assert l.dtype == np.int32 and c.dtype == np.int32
        assert list(zip(l.tolist(), c.tolist())) == ref_query_terms(want[s], lines, w), s
    assert [len(l) for l, _ in terms] == [1, 2, 0, 1]
