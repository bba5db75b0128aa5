"""The feature build and the query rows at every kernel form and form edge, with values that show the ORDER of a cell's
terms (feature_forms.py says how): the fp32 matrix against oracle.capi.index_features, the norms against capi.dot(1, x, x),
the query rows against a numpy fp64 restatement pinned to capi.finalize_query -- all as bytes.  -m gpu

  A  order probes between the lines of one pass, of three passes, of one turn of the prefetch ring, around a line that
     repeats a sample or descends, and at the tile edges of either accumulation kernel
  B  lines of exact lengths (register sets of line_prep_piece, pieces of 2048, the held and the chunked loop of
     line_flags_wave_kernel), breaks of the ascent and repeats at the hand-over points; the same repeats for
     line_flags_kernel (more than 65536 samples)
  C  sample counts at the edges of the flag forms: 65536 | 65537, 524288 | 524320 (64 KiB of bitmap), 2^20 | 2^20 + 32
  D  an item order of another length is ignored
  E  query rows of more than one tile of query_accumulate_kernel
  and ids outside [0, n_items), which build_features refuses before it launches anything
"""
import numpy as np
import pytest

import feature_forms as ff
from test_gpu_parity import _gpu_features

pytestmark = pytest.mark.gpu

ORDERS = [None, "ext", "reversed"]


def _build(f, order):
    keys, rp, s, c = f.arrays()
    a, prep = _gpu_features(keys, rp, s, c, f.sample_count, f.threshold, f.D, order)
    assert prep["n_items"] == f.n == a.get_n_items() and prep["ext_ids"].tolist() == f.ext.tolist()
    return a


def _blame(f, X):
    """What differs from the oracle: the count of cells, the probe groups hit, the named lines that touch such a cell."""
    ref = f.reference()["X"]
    rows, cols = np.nonzero(np.ascontiguousarray(X).view(np.uint32) != ref.view(np.uint32))
    out = ["%d cells differ" % len(rows)]
    out += ["probe group %s: %d of %d cells" % (t, f.changed(X, t), len(f.cells(t))) for t in f.tags() if f.changed(X, t)]
    names = getattr(f, "names", None)
    if names:                                   # the named lines are the first of lines[]; the roster follows them
        from oracle import capi
        buf, off = capi.pack_keys([f.lines[j][0] for j in range(len(names))])
        col = capi.hash_col_sign(buf, off, f.D)[1]
        bad = set(zip(f.ext[rows].tolist(), cols.tolist()))
        out += ["line '%s'" % names[j] for j in range(len(names)) if any((x, int(col[j])) in bad for x in f.lines[j][1].tolist())]
    return "; ".join(out)


def _check(f, a, norm_rows=None):
    from oracle import capi
    ref = f.reference()["X"]
    X = a.get_items()
    assert X.tobytes() == ref.tobytes(), _blame(f, X)
    rows = np.arange(f.n) if norm_rows is None else norm_rows
    want = np.array([capi.dot(1, ref[r], ref[r]) for r in rows], np.float32)
    assert a.get_norms2()[rows].tobytes() == want.tobytes()


# ----------------------------------------------------------------------------------------------------- A

@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("group", ["a", "b", "c", "d", "e"])
def test_order_probes(group, order):
    """(a) speaks of accumulate_piece_kernel (with the order), (b) of accumulate_kernel (without), (e) of both kernels'
    tiles; the other orders of those groups are the same file through the other kernel."""
    f = ff.order_file(group)
    _check(f, _build(f, order))


# ----------------------------------------------------------------------------------------------------- B

@pytest.mark.parametrize("order", ORDERS)
def test_exact_lengths_breaks_and_repeats(order):
    f = ff.lengths_file()
    _check(f, _build(f, order))


@pytest.mark.parametrize("order", ORDERS)
def test_repeats_with_a_workgroup_per_line(order):
    f = ff.wide_file()
    assert f.n > 65536
    _check(f, _build(f, order), norm_rows=np.concatenate([np.arange(0, f.n - 64, 97), np.arange(f.n - 64, f.n)]))


# ----------------------------------------------------------------------------------------------------- C

@pytest.mark.parametrize("order", [None, "ext"])
@pytest.mark.parametrize("n", ff.EDGE_COUNTS)
def test_sample_count_edges(n, order):
    """Both sides of 65536 samples (a bitmap per wave | per workgroup), of 64 KiB of bitmap and of 2^20 samples (no bitmap:
    every line that may repeat a sample is replayed).  The fused norm pass takes all of them: row counts that are no
    multiple of its 64 positions among them.

    524320 and 2^20 samples build as the library stood: line_flags_kernel's launch with more than 64 KiB of dynamic LDS
    (128 KiB at 2^20) is accepted on the MI355X without a raised limit."""
    f = ff.edge_file(n)
    _check(f, _build(f, order), norm_rows=np.concatenate([np.arange(0, n - 64, 4099), np.arange(n - 64, n)]))


# ----------------------------------------------------------------------------------------------------- D

def test_an_order_of_another_length_is_ignored():
    from morna_amd.annoy import AnnoyIndex
    from morna_amd.index import prepare_csr
    f = ff.order_file("d")
    keys, rp, s, c = f.arrays()
    prep = prepare_csr(keys, rp, s, c, f.sample_count, f.threshold)
    ref = f.reference()["X"]
    for key in (np.arange(f.n - 1), np.arange(f.n + 1), -np.arange(f.n + 1)):
        a = AnnoyIndex(f.D)
        a.stage_junctions(prep["key_bytes"], prep["key_off"], prep["row_ptr"], prep["ids"], prep["cov"], prep["idf"])
        a.stage_item_order(key)
        a.build_features(f.n)
        assert a.get_items().tobytes() == ref.tobytes(), len(key)
    a.stage_item_order(-np.asarray(prep["ext_ids"]))     # ... and one of the right length after a stale one is taken
    a.build_features(f.n)
    assert a.get_items().tobytes() == ref.tobytes()


# ----------------------------------------------------------------------------------------------------- E

@pytest.mark.parametrize("D", [8, 257])
@pytest.mark.parametrize("nq", [4096, 4097, 8200])
def test_query_rows_past_one_tile(nq, D):
    from morna_amd.annoy import AnnoyIndex
    from morna_amd.index import ParsedLines, pack_vocab
    L = ff.query_lines(nq, D)
    want = L["want64"]
    for q in sorted(set([0, 1, ff.QA_TILE - 1, ff.QA_TILE, 2 * ff.QA_TILE - 1, 2 * ff.QA_TILE, nq - 1]) & set(range(nq))):
        assert ff.finalize_row(q, L, D).tobytes() == want[q].tobytes(), q     # the restatement is the oracle's
    a = AnnoyIndex(D)
    a.add_items(np.ones((3, D), np.float32))
    terms = ParsedLines.from_arrays(L["prep"], L["sample_count"]).query_terms(pack_vocab(L["vocab"]), L["sample_count"])
    assert terms.n_lines == len(L["keys"]) and terms.nnz == len(L["prep"]["ids"])
    a.build_query_rows(terms)
    r64, r32 = a.get_query_rows()
    bad = np.nonzero((r64.view(np.uint64) != want.view(np.uint64)).any(axis=1))[0]
    assert r64.tobytes() == want.tobytes(), "rows %s ... differ (%d)" % (bad[:8].tolist(), len(bad))
    assert r32.tobytes() == want.astype(np.float32).tobytes()
    assert a.get_items().tobytes() == np.ones((3, D), np.float32).tobytes()


# ------------------------------------------------------------------------------------ ids outside the items

def test_ids_outside_the_items_are_refused():
    """The flag kernels index an LDS bitmap with the raw id: build_features refuses such lines on the host, from the range
    morna_stage_junctions recorded, and the handle builds the next, valid, lines as ever."""
    from morna_amd.annoy import AnnoyIndex
    from morna_amd.index import prepare_csr
    f = ff.order_file("c")
    keys, rp, s, c = f.arrays()
    prep = prepare_csr(keys, rp, s, c, f.sample_count, f.threshold)
    a = AnnoyIndex(f.D)
    for value, word in ((f.n, "largest"), (-1, "smallest")):
        ids = np.array(prep["ids"], np.int32)
        ids[len(ids) // 2] = value
        a.stage_junctions(prep["key_bytes"], prep["key_off"], prep["row_ptr"], ids, prep["cov"], prep["idf"])
        a.stage_item_order(prep["ext_ids"])
        with pytest.raises(IndexError, match=word):
            a.build_features(f.n)
        assert a.get_n_items() == 0
    a.stage_junctions(prep["key_bytes"], prep["key_off"], prep["row_ptr"], prep["ids"], prep["cov"], prep["idf"])
    a.build_features(f.n)
    assert a.get_items().tobytes() == f.reference()["X"].tobytes()
