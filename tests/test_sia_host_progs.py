"""The aligner's host-side stand-alone programs (tests/sia_host_progs.py; host code, AddressSanitizer and UBSan, no GPU).

sia_gate_cpu: csrc/sia_gate.h -- the one border test both of k_sia_run's patch loops and k_sia_precompute go through -- answers as the
reference's `(int) floorf` followed by the integer comparisons does on every in-range coordinate of its sweep (all floats within four ulps of
every gate, a dense sweep across each level, levels from 6 to 2^24 columns), and rejects NaN, the infinities, +-3e9 and the neighbours of 2^31,
where the reference's form is undefined and the GPU's saturating conversion would wrap past the gate.

sia_plan_cpu: what csrc/lds_layout.h decides for every case of tests/align_cases.py, proving that the cases take the kernel forms they are
meant for: the feature-count classes straddle the Jacobian terms' LDS limit (and k_sia_run's register form, 2 x 512 features), every level of
about 7 KB is staged in LDS, and the 509 x 331 level is not.  The kernel's static LDS enters as a bound read off its declarations; the value
recorded from the compiled kernel (tests/golden/lds_layout_parent.json) gives the same ceiling."""
from tests import align_cases as AC
from tests import lds_layout_prog, sia_host_progs

CASES = AC.cases()


def test_gate_header_equals_the_reference_form_and_rejects_what_it_leaves_undefined():
    assert int(sia_host_progs.run("sia_gate_cpu")) > 10 ** 7


def _launch(c):
    return len(c["keys"]), [int(c["cur_pyr"][l].shape[0] * c["cur_pyr"][l].shape[1]) for l in range(c["min_level"], c["max_level"] + 1)]


def test_lds_plan_of_every_case():
    recs = sia_host_progs.plans([_launch(c) for c in CASES])
    recorded = sia_host_progs.plans([_launch(c) for c in CASES], lds_layout_prog.golden()["aligner"]["static_lds"])
    assert [{k: v for k, v in r.items() if k != "static"} for r in recs] == [{k: v for k, v in r.items() if k != "static"} for r in recorded]
    assert recs[0]["static"] >= recorded[0]["static"]                     # the bound bounds the compiled kernel's
    by = {c["name"]: r for c, r in zip(CASES, recs)}
    assert all(r["fits"] and r["total"] <= r["ceiling"] for r in recs)
    # the feature-count classes: Jacobian terms in LDS up to 1755 features; the register form up to 2 x 512 (k_sia_run's kSiaBlock, not a layout matter)
    assert [by["count_%d" % n]["jac"] for n in AC.N_CLASSES] == [1, 1, 1, 0, 0]
    assert sorted(AC.N_CLASSES)[:2] == [1024, 1025]
    for c in CASES:
        r = by[c["name"]]
        if c["family"] == "unstaged":
            assert r["staged"] == [0] and c["cur_pyr"][0].size == 168479 and r["stage_bytes"] < 168479 + 8
        else:                                                              # levels of 7 KB and less: all staged, at every feature count
            assert all(r["staged"]) and max(_launch(c)[1]) <= 96 * 72 and r["stage_bytes"] >= max(_launch(c)[1]) + 8, c["name"]
    assert {len(by[n]["staged"]) for n in ("stale_a", "stale_c", "width_7")} == {3, 1}
