"""The numpy oracle of SvdDenoiser (tests/svd_denoiser_oracle.py) pinned on the reference's own checks (algorithm/test/qa_SvdFilter.cpp and
blocks/filter/test/qa_SvdDenoiser.cpp), and the cap on unsettled windows for every case the device test uses: at most 5 % of a case's windows may be skipped
there, and that is asserted here on the oracle alone."""
import numpy as np
import pytest

import svd_denoiser_oracle as SV


def test_defaults_are_the_blocks():
    d = SV.defaults("f32")  # SvdDenoiser.hpp:37-51
    assert (d["window_size"], d["hankel_rows"], d["max_rank"], d["energy_fraction"], d["hop_fraction"]) == (64, 0, 2**64 - 1, 1.0, 0.25)
    assert d["relative_threshold"] == d["absolute_threshold"] == float(np.finfo(np.float32).eps)
    assert SV.defaults("c64")["relative_threshold"] == float(np.finfo(np.float64).eps)


def test_hop_sizes_and_delays_of_the_reference():
    assert SV.derive("f32", window_size=32, hop_fraction=0.1)["hop"] == 3      # the product in float: 32 * 0.1f = 3.2000000477
    assert SV.derive("f64", window_size=32, hop_fraction=0.1)["hop"] == 3
    assert SV.derive("f64", window_size=64, hop_fraction=0.25)["hop"] == 16
    assert SV.derive("f32", window_size=32, hop_fraction=0.5)["hop"] == 16
    assert SV.derive("f64", window_size=32)["delay"] == 15 and SV.derive("f64", window_size=33)["delay"] == 16
    assert SV.derive("f32", window_size=1)["W"] == 2 and SV.derive("f32", window_size=64, hop_fraction=0.0)["hop"] == 1
    g = SV.derive("f32", window_size=33, hankel_rows=5, hop_fraction=1.0)
    assert (g["L"], g["K"], g["hop"], g["safe"]) == (5, 29, 33, 0)
    g = SV.derive("f32")
    assert (g["L"], g["K"], g["safe"]) == (32, 33, 32)


def test_rank_rule_walks_in_the_references_order():
    R = np.float64
    s = [4.0, 2.0, 1.0, 0.5]
    assert SV.effective_rank(s, R) == 4
    assert SV.effective_rank(s, R, max_rank=2) == 2
    assert SV.effective_rank(s, R, relative_threshold=0.3) == 2        # 1 / 4 < 0.3 stops before sigma_2
    assert SV.effective_rank(s, R, absolute_threshold=0.75) == 3
    assert SV.effective_rank(s, R, energy_fraction=0.75) == 1          # 16 / 21.25 >= 0.75: counted, then stop
    assert SV.effective_rank(s, R, energy_fraction=0.8) == 2
    assert SV.effective_rank(s, R, max_rank=0) == 1                    # max(rank, 1)
    assert SV.effective_rank([0.0, 0.0, 0.0], R) == 1                  # 0 / 0 compares false, the absolute threshold stops the walk
    assert SV.effective_rank([], R) == 0
    # float: the trailing sigma^2 is absorbed into the energy sum, so energy_fraction 1 stops early
    assert SV.effective_rank([1.0, 1e-5], np.float32) == 1 and SV.effective_rank([1.0, 1e-5], np.float64) == 2


def test_rank_one_matrix_and_full_energy_window_to_1e_10():
    w = 0.9 ** np.arange(16)  # a geometric window: its Hankel matrix has rank 1
    d, k, s = SV.low_rank_window(w, 8, np.float64, max_rank=1)
    assert k == 1 and np.max(np.abs(d - w)) <= 1e-10
    rng = np.random.default_rng(1)
    w = rng.standard_normal(32)
    d, k, s = SV.low_rank_window(w, 16, np.float64, energy_fraction=1.0)
    assert k == 16 and np.max(np.abs(d - w)) <= 1e-10


def test_near_dc_input_stays_within_a_tenth():
    x = 5.0 + 0.001 * np.sin(2 * np.pi * np.arange(200) / 50.0)
    r = SV.run(x, "f64", window_size=16, max_rank=2)
    assert np.all(np.isfinite(r.y)) and np.max(np.abs(r.y[32:] - 5.0)) <= 0.1


def test_noisy_sinusoid_comes_out_cleaner_than_it_went_in():
    n, fs = 512, 1000.0  # qa_SvdDenoiser.cpp:48-89, with its skip and delay
    rng = np.random.default_rng(42)
    clean = np.sin(2 * np.pi * 50.0 * np.arange(n) / fs)
    noisy = clean + 0.3 * rng.standard_normal(n)
    r = SV.run(noisy, "f64", window_size=64, max_rank=3, energy_fraction=0.95)
    delay = r.geom["delay"]
    skip = max(128, delay + 64)
    e_in = np.sqrt(np.mean((noisy[skip:] - clean[skip:]) ** 2))
    e_out = np.sqrt(np.mean((r.y[skip:] - clean[skip - delay:n - delay]) ** 2))
    assert e_out < e_in, (e_out, e_in)


@pytest.mark.parametrize("W", [2, 4])
def test_smallest_windows_are_finite(W):
    for dtype in ("f32", "f64"):
        r = SV.run(np.arange(20.0), dtype, window_size=W, max_rank=1)
        assert np.all(np.isfinite(r.y))
    r = SV.run(np.exp(0.3j * np.arange(20)), "c32", window_size=W)
    assert np.all(np.isfinite(r.y))


def test_all_zero_windows_are_settled_and_give_zeros():
    r = SV.run(np.zeros(100), "f32")
    assert r.unsettled() == 0 and not np.any(r.y) and all(w["k"] == 1 for w in r.windows)


def test_the_default_settings_are_the_delayed_identity():
    x, r = SV.case("B", "f64")
    delay = r.geom["delay"]
    # full rank windows reproduce the window, and d[safe] is the sample `delay` behind the newest
    assert np.max(np.abs(r.y[delay + 64:] - x[64:-delay])) <= 1e-12


@pytest.mark.parametrize("name,dtype", [(n, d) for n, c in SV.CASES.items() for d in c[2]])
def test_at_most_five_percent_of_a_cases_windows_are_unsettled(name, dtype):
    x, r = SV.case(name, dtype)
    print(f"{name} {dtype}: {r.unsettled()} of {len(r.windows)} windows unsettled")
    assert r.unsettled() <= 0.05 * len(r.windows), (r.unsettled(), len(r.windows))
    assert [w["start"] for w in r.windows] == list(range(0, x.size, r.geom["hop"]))
