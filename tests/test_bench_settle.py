"""bench.settle / timed_runs step bookkeeping (host logic, no GPU): the settle
phase replays whole 31-step batches from step 0, and the warm-up, the timed run
and the timing pass follow it on consecutive step indices."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class Rec:
    def __init__(self):
        self.calls = []

    def prepare_graphs(self):
        return 0.5

    def run(self, first, ctl, want_results=True):
        self.calls.append((first, len(ctl), want_results))
        return [{"resampled": 0}] * len(ctl) if want_results else None

    def enable_timing(self, on):
        pass

    def timing(self, k):
        return (0.0, 0)


def test_settle_whole_batches():
    r = Rec()
    ctl = np.zeros((100, 2))
    assert bench.settle(r.run, ctl, 65) == 62
    assert r.calls == [(0, 31, False), (31, 31, False)]
    assert bench.settle(Rec().run, ctl, 30) == 0


def test_timed_runs_step_indices_after_settle():
    r = Rec()
    settle, warm, steps = 62, 5, 20
    ctl = np.zeros((settle + warm + 2 * steps, 2))
    elapsed, out, timing, cap = bench.timed_runs(r, ctl, warm, steps, lambda: None,
                                                 settle_steps=settle)
    assert cap == 0.5 and len(out) == steps
    assert r.calls == [(0, 31, False), (31, 31, False), (62, 5, False), (67, 20, True), (87, 20, True)]


def test_timed_runs_plain_has_no_timing_pass():
    """kernel_timing=False (a plain bench run): settle, warm-up and the timed
    steps only; on_timed sees the filter and the timed run's records."""
    r = Rec()
    settle, warm, steps = 62, 5, 20
    ctl = np.zeros((settle + warm + steps, 2))
    seen = []
    elapsed, out, timing, cap = bench.timed_runs(r, ctl, warm, steps, lambda: None,
                                                 settle_steps=settle, kernel_timing=False,
                                                 on_timed=lambda f, o: seen.append((f, len(o))))
    assert timing is None and cap == 0.5 and len(out) == steps
    assert r.calls == [(0, 31, False), (31, 31, False), (62, 5, False), (67, 20, True)]
    assert seen == [(r, steps)]


def test_dump_outputs_files_and_fixed_sample(tmp_path, monkeypatch):
    """dump_outputs: one float64 .npy per record field and state array; a state
    above DUMP_STATE_MAX is written as the same sorted sample on every call."""
    rec = {"x_est": np.arange(3.0), "cov": np.eye(3), "max_val": 0.25, "max_idx": 7, "ess": 3.5,
           "weight_sum": 1e-30, "resampled": True, "resample_next": False, "status": 0}
    state = [np.arange(100.0) + k for k in range(4)]
    bench.dump_outputs(str(tmp_path / "all"), rec, state)
    got = {p.name[:-4]: np.load(p) for p in (tmp_path / "all").iterdir()}
    assert set(got) == {"x_est", "cov", "max_val", "max_idx", "ess", "weight_sum", "resampled",
                        "resample_next", "particles_x", "particles_y", "particles_th", "weights"}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["cov"].shape == (3, 3) and got["max_idx"].tolist() == [7.0]
    assert got["resampled"].tolist() == [1.0] and got["resample_next"].tolist() == [0.0]
    assert np.array_equal(got["particles_y"], state[1]) and np.array_equal(got["weights"], state[3])
    monkeypatch.setattr(bench, "DUMP_STATE_MAX", 16)
    for tag in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / tag), rec, state)
    x1, x2 = (np.load(tmp_path / t / "particles_x.npy") for t in ("s1", "s2"))
    assert x1.shape == (16,) and np.array_equal(x1, x2) and np.all(np.diff(x1) > 0)
    assert np.array_equal(np.load(tmp_path / "s1" / "weights.npy"), x1 + 3)


def test_index_error_row_reports_only_the_reference_index_error():
    """A --full row that reaches the reference's IndexError is reported in its
    place; a row that succeeds is returned as is; any other error propagates."""
    import pytest
    assert bench.index_error_row(lambda: {"value": 1.0}) == {"value": 1.0}

    def beyond():
        raise IndexError("resample position beyond the last cumulative weight; record 7")
    assert bench.index_error_row(beyond) == {
        "error": "IndexError: resample position beyond the last cumulative weight; record 7"}
    with pytest.raises(RuntimeError):
        bench.index_error_row(lambda: bench._raise(RuntimeError("hip error")))
