"""The helpers of the many-tile and wide-build junction-store tests (jstore_big.py) without a GPU: the planted structure of
the sparse stores, read from the restatements; the array form of ref_retain's answer against the list form the tile-edge
tests compare; the stable-sort statement of a built store against the dict-and-list one (test_junctions_cpu.sample_lists) on
the embedded files; and the lines of the wide build.  Integers and whole arrays."""
import numpy as np
import pytest

import jstore_big as big
from test_junctions_cpu import ref_retain, store_arrays, tiny_lines
from test_pool_cpu import ref_pool
from test_recovery_cpu import ref_hist


@pytest.mark.parametrize("n_lines", big.SIZES)
def test_planted_structure_and_the_restatements_at_many_tiles(n_lines):
    """The restatements loop in Python or allocate per line of the file: on these sparse rows each call takes well under a
    second at every size, so none needed a faster twin."""
    case = big.make_case(n_lines)
    rounds = big.check_planted(case)
    assert len(rounds) == -(-big.n_tiles(n_lines) // big.ROUND)
    rows, lists = case["rows"], case["lists"]
    # held by all: the every-seventh list under a frequency of 1 and a coverage nothing reaches keeps the planted lines
    lines, masks, cov_ptr, cov = big.retained_arrays(case, lists[3], 1.0, 2**40)
    assert set(big.planted_lines(n_lines)) <= set(lines.tolist()) and (masks == np.uint64(2**11 - 1)).all()
    assert cov_ptr.tolist() == list(range(0, 11 * len(lines) + 1, 11)) and cov[0] == -7
    # the pool of everything sums the three 2^31 - 1 past 32 bits; the histogram counts every line once
    held, sums, holders = ref_pool(rows, n_lines, case["groups"][4])
    at = int(np.searchsorted(held, big.BIG_LINE))
    assert held[at] == big.BIG_LINE and sums[at] >= 3 * big.BIG > 2**32 and holders[at] >= 3
    hist = ref_hist(rows, n_lines, lists[0], np.arange(n_lines), [1, 5, 50])
    assert hist[1].sum() == n_lines and hist[0].sum() == 0 and hist[1, 0, 0] > 8 * big.TILE


def test_retained_arrays_are_the_lists_of_the_tile_edge_tests():
    from morna_amd.junctions import Retained
    case = big.make_case(big.SIZES[0])
    rows, cov_at = case["rows"], case["cov_at"]
    for lst, f, c in ((case["lists"][4], 0.5, 3), (case["lists"][0], 0.0, 10**6), (case["lists"][1], 1.0, 1), ([], 0.5, 3)):
        got = Retained(*big.retained_arrays(case, lst, f, c))
        retained, found_in = ref_retain([rows[s][0].tolist() for s in lst], [rows[s][1].tolist() for s in lst], f, c)
        lines = sorted(retained)
        assert got.lines.tolist() == lines and got.found_in == [found_in[j] for j in lines]
        assert got.coverages == [[cov_at[lst[r]][j] for r in found_in[j]] for j in lines]
        assert (got.lines.dtype, got.masks.dtype, got._cov.dtype) == (np.int32, np.uint64, np.int32)


def lists_of_text(lines):
    samples = [np.array([int(x) for x in ln.strip().split("\t")[6].split(",")], np.int64) for ln in lines]
    covs = [np.array([int(x) for x in ln.strip().split("\t")[7].split(",")], np.int64) for ln in lines]
    return samples, covs


@pytest.mark.parametrize("which", ["generic", "tiny", "reversed"])
def test_expected_store_equals_sample_lists(which, embedded, tmp_path):
    """The stable sort by first-seen sample against the restatement of the reference's per-sample tables, and the file bytes
    against what the library saves for those arrays."""
    from morna_amd.junctions import JunctionStore
    lines = tiny_lines() if which == "tiny" else list(embedded["generic"])
    if which == "reversed":                                    # every line lists its samples in descending order
        rev = []
        for ln in lines:
            t = ln.rstrip("\n").split("\t")
            rev.append("\t".join(t[:6] + [",".join(reversed(t[6].split(","))), ",".join(reversed(t[7].split(",")))]) + "\n")
        lines = rev
    ext, ptr, line, cov, n_lines = store_arrays(lines)
    got = big.expected_store(*lists_of_text(lines))
    for a, b in zip(got, (ext, ptr, line, cov)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    path = str(tmp_path / "s.junc.mor")
    JunctionStore.from_arrays(ext, ptr, line, cov, n_lines).save(path)
    with open(path, "rb") as fh:
        assert fh.read() == big.store_file_bytes(*got, n_lines)


@pytest.mark.parametrize("S", big.WIDE_SIZES)
def test_wide_lines(S, tmp_path):
    samples, covs = big.wide_lines(S)
    assert len(samples) == big.WIDE_J == 40 and 16 <= big.ALL_LINE < 32 <= big.EDGE_LINE
    assert np.array_equal(np.sort(samples[big.ALL_LINE]), np.arange(S)) and not np.array_equal(samples[big.ALL_LINE], np.arange(S))
    assert all(len(np.unique(ids)) == len(ids) for ids in samples)             # no sample twice in a line
    ext, ptr, line, cov = big.expected_store(samples, covs)
    assert len(ext) == S and ptr[-1] == len(line) == sum(len(ids) for ids in samples)
    assert samples[big.EDGE_LINE].tolist() == ext[[S - 1, S - 32, S - 33, 0]].tolist() and ext[0] == samples[0][0]
    for s, c in zip((S - 1, S - 32, S - 33, 0), (big.BIG, 0, -5, -2**31)):     # the edge line's entries, found in the store
        mine = slice(ptr[s], ptr[s + 1])
        assert cov[mine][line[mine] == big.EDGE_LINE].tolist() == [c]
        assert (np.diff(line[mine]) > 0).all() and big.ALL_LINE in line[mine]
    if S == 262144:                                            # (S + 31) / 32 is the bitmap's 8192 words, the last bit its last
        assert ((S - 1) >> 5, (S - 1) & 31, (S - 32) >> 5, (S - 32) & 31, (S - 33) >> 5, (S - 33) & 31) == (8191, 31, 8191, 0, 8190, 31)
    assert (S + 31) // 32 == (8192 if S == 262144 else 8193)
    ids, c = big.with_repeat(samples[33], covs[33], int(ext[S - 1]))
    assert (ids == ext[S - 1]).sum() == 2 and len(ids) == len(c)
    path = str(tmp_path / "wide.tsv.gz")
    big.write_lines(path, samples[:3], covs[:3])
    import gzip
    with gzip.open(path, "rt") as fh:
        text = fh.readlines()
    assert [a.tolist() for a in lists_of_text(text)[0]] == [a.tolist() for a in samples[:3]]
    assert [a.tolist() for a in lists_of_text(text)[1]] == [a.tolist() for a in covs[:3]]
    assert len(set(" ".join(ln.split("\t")[:3]) for ln in text)) == 3
