"""Batch queries from an intropolis file, host side (no GPU): the native pre-pass morna_lines_query_terms against a
plain-Python restatement of the contract, the rows it implies against MornaSearch.finalize_query and the oracle, and the
command line's flag checks.

The contract: for query sample s, every line listing s, in file order, fed as the raw junction (chrom, start, end,
coverage of s) through cli.py's `if key in sample_frequencies: update_query(...)` filter, then finalize_query."""
import gzip
import math
import os
from collections import defaultdict
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN


def _open(path):
    return gzip.open(path, "rt") if str(path).endswith(".gz") else open(path)


def query_terms(path, freq, sample_count):
    """The native pre-pass: the query file parsed with threshold 0, then its terms against the vocabulary `freq`."""
    from morna_amd.index import ParsedLines, pack_vocab
    parsed = ParsedLines(str(path), sample_count=sample_count, sample_threshold=0)
    return parsed.query_terms(pack_vocab(freq), sample_count)


def restate(path, freq, sample_count):
    """The pre-pass in plain Python: (first-seen external ids, [[key, [ext ids], [coverage sums], weight], ...])."""
    from morna_amd.index import tokenize_line
    ext_ids, seen, out, first = [], {}, [], {}
    with _open(path) as fh:
        for line in fh:
            key, samples, covs = tokenize_line(line)
            pairs = list(zip(samples, covs))
            for s, _ in pairs:
                if s not in seen:
                    seen[s] = len(ext_ids)
                    ext_ids.append(s)
            if key not in freq:
                continue
            df = freq[key]
            entry = [key, [], [], math.log(float(sample_count) / df) if df else 0.0]
            for s, c in pairs:
                if (key, s) in first:
                    e, i = first[(key, s)]
                    e[2][i] += c
                else:
                    first[(key, s)] = (entry, len(entry[1]))
                    entry[1].append(s)
                    entry[2].append(c)
            if entry[1]:
                out.append(entry)
    return ext_ids, out


def terms_as_lists(T):
    a = T.arrays()
    kb, ko, rp = a["key_bytes"].tobytes(), a["key_off"], a["row_ptr"]
    ext = a["ext_ids"]
    lines = []
    for j in range(T.n_lines):
        ids = a["ids"][rp[j]:rp[j + 1]]
        lines.append([kb[ko[j]:ko[j + 1]].decode("ascii"), ext[ids].tolist(), a["cov"][rp[j]:rp[j + 1]].tolist(), a["idf"][j]])
    return ext.tolist(), lines


def densify(T, dim):
    """fp64 rows [nq, dim] of the pre-pass output, walked in its line order: row[id][col] += sign * (cov * w)."""
    import ctypes as C
    from morna_amd._lib import lib
    a = T.arrays()
    kb, ko, rp = a["key_bytes"].tobytes(), a["key_off"], a["row_ptr"]
    rows = np.zeros((T.n_items, dim), np.float64)
    for j in range(T.n_lines):
        key = kb[ko[j]:ko[j + 1]]
        h = int(lib().morna_hash32(C.c_char_p(key), len(key)))
        ids = a["ids"][rp[j]:rp[j + 1]]
        term = a["cov"][rp[j]:rp[j + 1]].astype(np.float64) * a["idf"][j]
        if h < 0:
            term = -term
        rows[ids, h % dim] = rows[ids, h % dim] + term        # a line lists a sample once
    return rows


def finalize_rows(path, freq, sample_count, dim, ext_ids):
    """MornaSearch.update_query / finalize_query (called unbound) for every sample, fed as `search -f raw` feeds it."""
    from morna_amd.search import MornaSearch
    ns = {s: SimpleNamespace(query=defaultdict(int), sample_frequencies=freq, sample_count=sample_count, dim=dim)
          for s in ext_ids}
    with _open(path) as fh:
        for line in fh:
            tokens = line.strip().split('\t')
            for s, c in zip([int(x) for x in tokens[-2].split(',')], [int(x) for x in tokens[-1].split(',')]):
                junction = (tokens[0], int(tokens[1]), int(tokens[2]), c)
                if " ".join(str(_) for _ in junction[:3]) in freq:
                    MornaSearch.update_query(ns[s], junction)
    rows = np.zeros((len(ext_ids), dim), np.float64)
    for q, s in enumerate(ext_ids):
        MornaSearch.finalize_query(ns[s])
        rows[q] = ns[s].query_sample
    return rows, ns


def check_all(path, freq, sample_count, dims):
    T = query_terms(path, freq, sample_count)
    ext, lines = restate(path, freq, sample_count)
    got_ext, got = terms_as_lists(T)
    assert got_ext == ext
    assert len(got) == len(lines)
    for g, w in zip(got, lines):
        assert g[:3] == w[:3]
        assert np.float64(g[3]).tobytes() == np.float64(w[3]).tobytes(), (g[0], g[3], w[3])   # bit-identical to math.log
    from oracle import capi
    capi.build()
    for dim in dims:
        rows = densify(T, dim)
        want, ns = finalize_rows(path, freq, sample_count, dim, ext)
        assert rows.tobytes() == want.tobytes(), dim
        for q, s in enumerate(ext):
            keys = [" ".join(map(str, k)) for k in ns[s].query]
            if not keys:
                assert not rows[q].any()
                continue
            o = capi.finalize_query(keys, list(ns[s].query.values()), [freq.get(k, 0) for k in keys], sample_count, dim)
            assert o.tobytes() == rows[q].tobytes(), (dim, s)
    return T, ext


CRAFTED = [
    # key A: samples 10, 20
    ("chr1", 100, 200, "10,20", "3,4"),
    # key B (the same column as A when dim is 1)
    ("chr2", 10, 20, "20,30", "1,2"),
    # key A again: 10 shared with its first line, 30 not (A's first line lacks 30, B lies in between)
    ("chr1", 100, 200, "10,30", "5,6"),
    # outside the vocabulary: sample 40 has no vocabulary key at all
    ("chr9", 1, 1, "40", "9"),
    # a sample repeated within a line
    ("chr3", 1, 2, "50,50,20", "1,2,3"),
    # key B again: only a sample it holds already
    ("chr2", 10, 20, "20", "7"),
    # samples out of order; then a key of frequency 0 (weight 0)
    ("chrX", 5, 9, "30,10", "2,2"),
    ("chr5", 7, 8, "60,10", "4,4"),
    # a line whose zip() truncates
    ("chr3", 1, 2, "70,10,20", "8,1"),
]
CRAFTED_FREQ = {"chr1 100 200": 5, "chr2 10 20": 2, "chr3 1 2": 7, "chrX 5 9": 1, "chr5 7 8": 0, "chr7 1 1": 4}


def write_crafted(path, lines):
    with (gzip.open(path, "wt") if str(path).endswith(".gz") else open(path, "w")) as fh:
        for c, s, e, samples, covs in lines:
            fh.write("%s\t%d\t%d\t+\tGT\tAG\t%s\t%s\n" % (c, s, e, samples, covs))


@pytest.mark.parametrize("gz", [False, True])
def test_crafted_query_file(tmp_path, gz):
    path = tmp_path / ("q.tsv.gz" if gz else "q.tsv")
    write_crafted(path, CRAFTED)
    T, ext = check_all(path, CRAFTED_FREQ, 11, [1, 2, 3, 128])
    assert ext == [10, 20, 30, 40, 50, 60, 70]
    # the merges happened: A holds 10 (3 + 5), 20 and, on its second line, 30 alone; B's last line is gone
    _, lines = terms_as_lists(T)
    assert [ln[0] for ln in lines] == ["chr1 100 200", "chr2 10 20", "chr1 100 200", "chr3 1 2", "chrX 5 9", "chr5 7 8",
                                       "chr3 1 2"]
    assert lines[0][1:3] == [[10, 20], [8, 4]]
    assert lines[1][1:3] == [[20, 30], [8, 2]]
    assert lines[2][1:3] == [[30], [6]]
    assert lines[3][1:3] == [[50, 20], [3, 3]]
    assert lines[6][1:3] == [[70, 10], [8, 1]]
    assert lines[5][3] == 0.0
    rows = densify(T, 3)
    assert not rows[ext.index(40)].any()                        # no vocabulary junction: a zero row, still a query


def test_golden_tiny_file(tmp_path):
    from morna_amd.index import ParsedLines
    path = os.path.join(GOLDEN, "tiny_intropolis.tsv")
    freq = ParsedLines(path, sample_count=6850, sample_threshold=100).frequencies()
    assert freq
    T, ext = check_all(path, freq, 6850, [128, 3000])
    assert T.n_items == len(ext) > 100


def test_random_query_file_with_duplicates(tmp_path):
    """Many duplicate-key lines, repeats inside lines and keys outside the vocabulary, at random."""
    rng = np.random.default_rng(5)
    keys = [("chr%d" % rng.integers(1, 4), int(rng.integers(1, 60)), int(rng.integers(60, 90))) for _ in range(40)]
    lines = []
    for _ in range(300):
        c, s, e = keys[int(rng.integers(0, len(keys)))]
        n = int(rng.integers(1, 8))
        samples = rng.integers(1, 25, size=n)
        lines.append((c, s, e, ",".join(map(str, samples)), ",".join(str(int(x)) for x in rng.integers(-3, 50, size=n))))
    freq = {"%s %d %d" % k: int(rng.integers(0, 30)) for k in keys[:30]}
    path = tmp_path / "r.tsv"
    write_crafted(path, lines)
    check_all(path, freq, 29, [1, 5, 64])


def test_coverage_sum_past_int32_is_rejected(tmp_path):
    path = tmp_path / "big.tsv"
    write_crafted(path, [("chr1", 100, 200, "10,20", "2147483000,5"), ("chr2", 10, 20, "10", "9"),
                         ("chr1", 100, 200, "10", "648")])
    with pytest.raises(ValueError, match=r"sample 10 at junction 'chr1 100 200' sums to 2147483648"):
        query_terms(path, CRAFTED_FREQ, 11)
    # one below the limit is kept
    write_crafted(path, [("chr1", 100, 200, "10,20", "2147483000,5"), ("chr1", 100, 200, "10", "647")])
    T = query_terms(path, CRAFTED_FREQ, 11)
    assert T.arrays()["cov"].tolist() == [2147483647, 5]


def test_vocabulary_and_sample_count_checks(tmp_path):
    from morna_amd.index import ParsedLines, pack_vocab
    path = tmp_path / "q.tsv"
    write_crafted(path, CRAFTED)
    parsed = ParsedLines(str(path), sample_count=11, sample_threshold=0)
    with pytest.raises(ValueError, match="sample count must be positive"):
        parsed.query_terms(pack_vocab(CRAFTED_FREQ), 0)
    kb, ko, df = pack_vocab({"chr1 100 200": 3, "chr2 10 20": 1})
    with pytest.raises(ValueError, match="repeats a key"):
        parsed.query_terms((np.concatenate([kb, kb]), np.concatenate([ko, ko[1:] + ko[-1]]), np.concatenate([df, df])), 11)
    T = parsed.query_terms(pack_vocab({}), 11)                   # an empty vocabulary: every query has the zero row
    assert T.n_lines == 0 and T.n_items == 7


@pytest.mark.parametrize("argv", [
    ["--intropolis", "q.tsv", "--query-ids", "1,2"],
    ["--intropolis", "q.tsv", "-q", "3"],
    ["--intropolis", "q.tsv", "-c", "5"],
    ["--intropolis", "q.tsv", "-rl"],
    ["--query-ids", "1,2", "-q", "3"],
    ["--query-ids", "1", "-c", "2"],
    ["--query-ids", "1", "-rl"],
    ["--query-ids", "1,x"],
])
def test_cli_rejects_batch_flag_combinations(tmp_path, capsys, argv):
    """An argparse error (exit status 2) before the index is read: the basename does not even exist."""
    from morna_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["search", "-x", str(tmp_path / "no_such_index")] + argv)
    assert e.value.code == 2
    assert "error:" in capsys.readouterr().err
