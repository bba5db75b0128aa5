"""A plain-Python restatement of the explain contract: dicts, float products (one rounding per
operation, as Python's float is fp64) and sums in the stated order.  The yardstick of test_explain_cpu.py and of the GPU
tests; no numpy arithmetic, no GPU."""
import struct
from math import sqrt

SUMS = ("pq", "pp", "qq", "pp_shared", "qq_shared", "distance")
COUNTS = ("shared", "n_q", "n_r")


def explain_pair(q_lines, q_cov, r_lines, r_cov, w, top):
    """The pair (query, result row), each ascending lines with their coverages, under the weights w: a dict of SUMS and
    COUNTS, and "lines", "terms", "cov_r": the top list."""
    vq = {}
    qq, n_q = 0.0, 0
    for l, c in zip(q_lines, q_cov):
        v = float(int(c)) * float(w[int(l)])
        vq[int(l)] = v
        qq = qq + v * v
        n_q += 1 if v != 0.0 else 0
    pq = pp = pp_shared = qq_shared = 0.0
    shared = n_r = 0
    entries = []
    for l, c in zip(r_lines, r_cov):
        l, c = int(l), int(c)
        v_r = float(c) * float(w[l])
        v_q = vq.get(l, 0.0)
        term = v_r * v_q
        pq = pq + term
        pp = pp + v_r * v_r
        pp_shared = pp_shared + (v_r * v_r if v_q != 0.0 else 0.0)
        qq_shared = qq_shared + (v_q * v_q if v_r != 0.0 else 0.0)
        n_r += 1 if v_r != 0.0 else 0
        if v_r != 0.0 and v_q != 0.0:
            shared += 1
            entries.append((term, l, c))
    ppqq = pp * qq
    radicand = 2.0 - 2.0 * pq / sqrt(ppqq) if ppqq > 0 else 2.0
    best = sorted(entries, key=lambda e: (-e[0], e[1]))[:min(int(top), shared)]
    return dict(pq=pq, pp=pp, qq=qq, pp_shared=pp_shared, qq_shared=qq_shared, distance=sqrt(max(radicand, 0.0)), shared=shared,
                n_q=n_q, n_r=n_r, lines=[e[1] for e in best], terms=[e[0] for e in best], cov_r=[e[2] for e in best])


def bits(x):
    """The 8 bytes of a float."""
    return struct.pack("<d", float(x))


def assert_pair(got, want, what=""):
    """An Explained (or anything with its attributes) against explain_pair's dict, byte for byte."""
    for name in SUMS:
        assert bits(getattr(got, name)) == bits(want[name]), "%s %s: %r != %r" % (what, name, getattr(got, name), want[name])
    for name in COUNTS:
        assert int(getattr(got, name)) == want[name], "%s %s: %r != %r" % (what, name, getattr(got, name), want[name])
    assert [int(x) for x in got.lines] == want["lines"], "%s lines" % what
    assert [int(x) for x in got.cov_r] == want["cov_r"], "%s cov_r" % what
    assert [bits(x) for x in got.terms] == [bits(x) for x in want["terms"]], "%s terms" % what
