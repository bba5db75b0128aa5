"""The generators of test_gpu_feature_forms.py (feature_forms.py) checked from the oracle alone: the order probes
distinguish, the wrong walks they are planted for change them, the planted lines are what their names say, and the numpy
restatement of the query rows is capi.finalize_query's."""
import numpy as np
import pytest

import feature_forms as ff


@pytest.mark.parametrize("group", ["a", "b", "c", "d", "e"])
def test_order_probes_distinguish(group):
    """check_probes ran when the file was made (a quarter of the planted cells, 8 per group); here: what it found."""
    f = ff.order_file(group)
    planted = sum(v[0] for v in f.kept.values())
    assert planted == len(f.cells()) >= 48 and all(v[1] >= 8 for v in f.kept.values())
    assert f.changed(f.reference()["X"]) == 0


def test_wrong_walks_change_the_probes():
    """The orders a wrong kernel would take, as permutations of the file given to the oracle."""
    a, b = ff.order_file("a"), ff.order_file("b")
    X = a.oracle(a.reordered(ff.reverse_inside_passes(ff.AW_LINES)))["X"]
    assert a.changed(X, "a-same") >= 8 and a.changed(X, "a-edge") >= 8
    X = a.oracle(a.reordered(ff.passes_last_to_first(ff.AW_LINES)))["X"]
    assert a.changed(X, "a-three") >= 8 and a.changed(X, "a-edge") >= 8
    X = b.oracle(b.reordered(ff.passes_last_to_first(ff.ACC_LINES)))["X"]
    assert b.changed(X, "b-three") >= 8 and b.changed(X, "b-edge") >= 8 and b.changed(X, "b-same") == 0
    X = b.oracle(b.reordered(ff.reverse_inside_passes(ff.ACC_LINES)))["X"]
    assert b.changed(X, "b-same") >= 8
    X = b.oracle(b.reordered(ff.reverse_inside_passes(ff.ACC_PFD)))["X"]
    assert b.changed(X, "b-ring") >= 8
    # the usual values do not show any of this: the whole of test_gpu_parity's synthetic file, its lines reversed
    from oracle import capi
    from test_gpu_parity import _synthetic_lines
    keys, rp, s, c = _synthetic_lines(np.random.default_rng(8675309 + 64), 700, 1500, 5, 120, dup_keys=False, weird=False)
    buf, off = capi.pack_keys(keys)
    fwd = capi.index_features(buf, off, rp, s, c, 700, 20, 64)
    rev = np.arange(len(keys))[::-1]
    lens = np.diff(rp)
    at = np.concatenate([np.arange(rp[j], rp[j + 1]) for j in rev])
    rp2 = np.zeros(len(keys) + 1, np.int64)
    np.cumsum(lens[rev], out=rp2[1:])
    buf2, off2 = capi.pack_keys([keys[j] for j in rev])
    bwd = capi.index_features(buf2, off2, rp2, s[at], c[at], 700, 20, 64)
    assert fwd["X"][np.argsort(fwd["ext_ids"])].tobytes() == bwd["X"][np.argsort(bwd["ext_ids"])].tobytes()


def test_planted_lines_are_what_they_say():
    f = ff.lengths_file()
    assert f.n >= 4200 and f.D == 24 and f.reference()["n_items"] == f.n
    lens = {name: len(f.lines[j][1]) for j, name in enumerate(f.names)}
    assert [lens["len %d" % L] for L in ff.EXACT_LENGTHS] == list(ff.EXACT_LENGTHS)
    for j, name in enumerate(f.names):
        s = f.lines[j][1]
        if name.startswith("len") and "repeat" not in name and "break" not in name:
            assert (np.diff(s) > 0).all(), name
        if "break" in name:
            k = int(name.split()[-1])
            assert s[k] < s[k - 1] and (s[k - 1] > ff.AW_TILE) != (s[k] > ff.AW_TILE), name
        if "entries in tile 0" in name:
            assert (s <= ff.AW_TILE).sum() == int(name.split()[0]) and (np.diff(s) > 0).all(), name
    for L in ff.PLANT_LENGTHS:
        for name, pairs in ff.repeat_plants(L).items():
            s = f.lines[f.names.index("len %d repeat %s" % (L, name))][1]
            assert len(s) == L and all(s[i] == s[k] for i, k in pairs), name
    assert set(ff.repeat_plants(2649)) == {"63|64", "0|last", "two in 0..63", "5|5+2048", "2053|2054"}
    assert "5|5+2048" not in ff.repeat_plants(2048)
    w = ff.wide_file()
    assert w.n == 66000 and w.D == 8
    assert {"0|1023", "0|1024", "1024|1025", "3|1024", "5|5+2048"} <= set(ff.repeat_plants(2100, wide=True))
    assert "0|1024" not in ff.repeat_plants(1024, wide=True) and "0|1023" in ff.repeat_plants(1024, wide=True)


@pytest.mark.parametrize("n", [ff.EDGE_COUNTS[1], ff.EDGE_COUNTS[-1]])
def test_edge_files_cover_every_sample(n):
    f = ff.edge_file(n)
    assert f.reference()["n_items"] == n and f.kept["edge"][1] >= 8
    assert 1 <= len(f.order) - (n + 3499) // 3500 <= 100 and max(len(ln[1]) for ln in f.lines) <= 3500


@pytest.mark.parametrize("nq,D", [(4097, 8), (8200, 257)])
def test_query_restatement_is_finalize_query(nq, D):
    L = ff.query_lines(nq, D)
    rp, ids = L["rp"], L["prep"]["ids"]
    lens = np.diff(rp)
    assert {1, 255, 256, 257}.issubset(lens.tolist()) and lens.max() >= min(3000, nq - ff.QA_TILE)
    second = [j for j in range(len(lens)) if ids[rp[j]:rp[j + 1]].min() >= ff.QA_TILE]
    astride = [j for j in range(len(lens)) if {ff.QA_TILE - 1, ff.QA_TILE} <= set(ids[rp[j]:rp[j + 1]].tolist()) and lens[j] > 256]
    assert second and astride and (nq < 8000 or max(lens[j] for j in second) > 256)
    for q in (0, ff.QA_TILE - 1, ff.QA_TILE, nq - 1):
        assert ff.finalize_row(q, L, D).tobytes() == L["want64"][q].tobytes()
