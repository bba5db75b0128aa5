"""The restatement of the two_means dispatch that test_gpu_width_forms.py expects launch counts from (width_forms.py,
tm_form), against widths written out by hand from forest_host.hpp (fb_attempt): float4 per lane = ceil(f / 256);
strips for 4, 8, 12, 16 ... 32 of them while a level has at most 2 * n_cus nodes; one wave for 1, 2, 3, 4, 6, 8, 12;
the wide form past 8192 floats whatever the switches, unrolled for 12, 16, 24 or 32 groups of four k-steps; else LDS.

And the restatement of the search's dispatch over the row width (width_forms.py, descent_nv), against widths written out by
hand from knn.hip (row_nv, with_row_nv): register forms of 1, 2, 3, 4, 6, 8, 12, 16, 24 and 32 float4 per lane, of which a
call site builds those up to its bound (32: the plain and the restricted descent; 12: the sweep descent and the root
margins by query groups); every other width takes the register-free form 0.
"""
import pytest

import width_forms as wf


@pytest.mark.parametrize("f,A,strip_on,want", [
    (1, 1, True, ("wave", 1)), (256, 9000, True, ("wave", 1)), (257, 4, True, ("wave", 2)),
    (641, 8, True, ("wave", 3)), (768, 8, True, ("wave", 3)),
    (769, 8, True, ("strip", 4)), (1000, 512, True, ("strip", 4)), (1000, 513, True, ("wave", 4)),
    (1000, 8, False, ("wave", 4)),
    (1100, 4, True, ("lds", None)), (1280, 4, False, ("lds", None)),
    (1500, 4, True, ("wave", 6)), (1537, 4, True, ("lds", None)),
    (2000, 4, True, ("strip", 8)), (2000, 600, True, ("wave", 8)), (2000, 4, False, ("wave", 8)),
    (2303, 2, True, ("lds", None)), (2560, 2, True, ("lds", None)),
    (3000, 400, True, ("strip", 12)), (3000, 1600, True, ("wave", 12)), (3000, 2, False, ("wave", 12)),
    (3073, 2, True, ("lds", None)),
    (4096, 2, True, ("strip", 16)), (4096, 513, True, ("lds", None)), (4096, 2, False, ("lds", None)),
    (4097, 2, True, ("lds", None)),                                  # 17 float4 per lane: no strip form
    (5000, 2, True, ("strip", 20)), (5900, 3, True, ("strip", 24)), (7000, 2, True, ("strip", 28)),
    (7800, 2, True, ("lds", None)), (8192, 2, True, ("strip", 32)), (8192, 2, False, ("lds", None)),
    (8193, 2, True, ("wide", 12)), (8193, 2, False, ("wide", 12)), (12288, 2, True, ("wide", 12)),
    (12289, 9000, True, ("wide", 12)),                               # 49 k-steps: 12 full groups of four and a tail
    (13312, 2, True, ("wide", 16)), (16384, 2, True, ("wide", 16)), (17500, 2, True, ("wide", 24)),
    (24832, 2, False, ("wide", 24)), (25600, 2, True, ("wide", 32)), (32768, 1, True, ("wide", 32))])
def test_tm_form_restates_the_dispatch(f, A, strip_on, want):
    assert wf.tm_form(f, A, 256, strip_on) == want
    assert wf.tm_timer(want[0]) == ("tm_strip" if want[0] in ("strip", "wide") else "tm_wave")


def test_tm_form_follows_the_device_size():
    """Strips while a level's nodes fit the chip twice over: the bound moves with the compute units."""
    assert wf.tm_form(3000, 200, 100) == ("strip", 12) and wf.tm_form(3000, 201, 100) == ("wave", 12)
    assert wf.expected_timers(1000, {0: 150, 1: 300, 2: 600, 3: 1200}, 256) == {"tm_strip": 2, "tm_wave": 2}
    assert wf.expected_timers(1000, {0: 150, 1: 300, 2: 600, 3: 1200}, 256, strip_on=False) == {"tm_strip": 0, "tm_wave": 4}
    assert wf.expected_timers(17500, {0: 2}, 256, strip_on=False) == {"tm_strip": 1, "tm_wave": 0}


@pytest.mark.parametrize("f,want32,want12", [
    (1, 1, 1), (64, 1, 1), (256, 1, 1), (257, 2, 2), (500, 2, 2), (641, 3, 3), (768, 3, 3), (769, 4, 4), (1000, 4, 4),
    (1025, 0, 0), (1100, 0, 0), (1280, 0, 0), (1281, 6, 6), (1300, 6, 6), (1500, 6, 6), (1537, 0, 0), (1793, 8, 8),
    (2000, 8, 8), (2049, 0, 0), (2303, 0, 0), (2817, 12, 12), (3000, 12, 12), (3072, 12, 12), (3073, 0, 0),
    (3841, 16, 0), (4096, 16, 0), (4097, 0, 0), (5000, 0, 0), (5889, 24, 0), (5900, 24, 0), (6144, 24, 0), (6145, 0, 0),
    (7000, 0, 0), (7800, 0, 0), (7937, 32, 0), (8192, 32, 0), (8193, 0, 0), (17500, 0, 0), (32768, 0, 0)])
def test_descent_nv_restates_the_dispatch(f, want32, want12):
    assert wf.descent_nv(f, 32) == want32 and wf.descent_nv(f, 12) == want12
