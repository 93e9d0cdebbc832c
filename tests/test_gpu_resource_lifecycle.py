"""The device buffers, page-locked buffers, events and streams a context and a sampler keep (csrc/sepaihrd_host_util.h: every one
has an owner that releases it): buffers that grow on the way and are reused larger than needed afterwards give what a fresh
object gives for the same call, bit for bit, and objects are created and destroyed in turn without leaving anything behind
that changes the next one's results.  Smallest fixture of the suite, production (fma) arithmetic."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHAINS, ITERS, THIN, BURN, PERIOD, SEED = 4, 24, 2, 4, 6, 17


def _same(got, fresh, what):
    assert got.keys() == fresh.keys()
    for key in fresh:
        assert np.array_equal(got[key], fresh[key], equal_nan=True), (what, key)


def test_context_buffers_grow_and_are_reused(mm, synth400):
    """Staging, results slab and its page-locked mirror, workspace and trajectory buffer: B = 3, then 70 with trajectories (all
    grow), then 5 with trajectories (all larger than needed); the finite-difference buffers of both contexts: 2 rows, 9, 2."""
    pb = synth400.with_(arith=mm.ARITH_FMA)
    theta = mm.draws.jitter_draws(pb, 11, 70)
    calls = [lambda h: h.eval_batch(theta[:3]),
             lambda h: h.eval_batch(theta, want_traj=True),
             lambda h: h.eval_batch(theta[3:8], want_traj=True),
             lambda h: h.fd_gradient_batch(theta[:2]),
             lambda h: h.fd_gradient_batch(theta[10:19]),
             lambda h: h.fd_gradient_batch(theta[5:7])]
    shared = mm.HipObjective(pb)
    for i, call in enumerate(calls):
        fresh = mm.HipObjective(pb)
        _same(call(shared), call(fresh), i)
        fresh.close()
    assert (shared.eval_batch(theta[:3])["status"] == 0).any()
    shared.close()


class _Sampler:
    """One context with one sampler on it, stepped as MultiChainMetropolisHastings steps a device-resident run: the chains'
    streams and the scale adaptation on the device where the libm self-check allows it (the sampler then only queues
    iterations), else the test's inputs drawn here with a fixed seed and fed through the page-locked buffers."""

    def __init__(self, mm, pb, x0, cov0):
        self.lib, self.P = mm.hipabi.load_library(), pb.n_params
        self.hip = mm.HipObjective(pb)
        self.device_streams = self.hip.device_libm_check() == (0, 0)
        self.mh = mm.hipabi.mh_create(self.lib, self.hip.ctx, CHAINS, ITERS, x0, cov0, thinning=THIN)
        assert self.mh, self.lib.sepaihrd_last_error(self.hip.ctx)
        self.rng = np.random.default_rng(SEED)
        self.done = 0  # accept tests so far: the history holds 1 + done states
        lib, mh, ones = self.lib, self.mh, np.ones(CHAINS)
        lp, st = np.empty(CHAINS), np.empty(CHAINS, dtype=np.int32)
        self._ok(lib.sepaihrd_mh_evaluate_current(mh, lp.ctypes.data, st.ctypes.data))
        lp = np.where((st >= 2) | ~np.isfinite(lp), -1e18, lp)
        if self.device_streams:
            self._ok(lib.sepaihrd_mh_keep_scale_on_device(mh, 1, 0.234, 0))
        self._ok(lib.sepaihrd_mh_set_values(mh, lp.ctypes.data))
        if self.device_streams:
            self._ok(lib.sepaihrd_mh_seed_streams(mh, SEED))
            self._ok(lib.sepaihrd_mh_draw_first(mh))
        else:
            self._stage()
        self._ok(lib.sepaihrd_mh_step(mh, None, ones.ctypes.data, None, None, 0, 10.0 / 101.0, self._adapt(1)))

    def _ok(self, rc):
        assert rc == 0, (rc, self.lib.sepaihrd_last_error(self.hip.ctx))

    @staticmethod
    def _adapt(t):
        return 0 if t <= BURN else 1 if t % PERIOD else 2

    def _pinned(self, address, count):
        return np.ctypeslib.as_array((C.c_double * count).from_address(address))

    def _stage(self):
        buf = self._pinned(self.lib.sepaihrd_mh_staging_buffer(self.mh), CHAINS * self.P)
        buf[:] = self.rng.standard_normal(CHAINS * self.P)
        self._ok(self.lib.sepaihrd_mh_stage_normals(self.mh, buf.ctypes.data))

    def advance(self, done):
        """accept test, commit and next proposal, until `done` tests have been made"""
        lib, mh = self.lib, self.mh
        while self.done < done:
            t = self.done + 1
            last = 1 if t + 1 >= ITERS else 0
            if not self.device_streams:
                tb = self._pinned(lib.sepaihrd_mh_test_buffer(mh), 3 * CHAINS + CHAINS * self.P)
                tb[:CHAINS] = np.log(self.rng.uniform(size=CHAINS))
                tb[CHAINS:3 * CHAINS] = 1.0
                tb[3 * CHAINS:] = self.rng.standard_normal(CHAINS * self.P)
                if not last:
                    self._stage()
            self._ok(lib.sepaihrd_mh_step_tested(mh, 10.0 / ((t + 1) + 100.0), self._adapt(t + 1), last))
            if not self.device_streams:
                values, flags = np.empty(CHAINS), np.empty(CHAINS, dtype=np.uint8)
                self._ok(lib.sepaihrd_mh_fetch_test(mh, values.ctypes.data, flags.ctypes.data))
            self.done = t

    def history(self, rows):
        rows = np.asarray(rows, dtype=np.int32)
        out = np.empty((CHAINS, len(rows), self.P))
        self._ok(self.lib.sepaihrd_mh_read_history(self.mh, rows.ctypes.data, len(rows), out.ctypes.data))
        return {"history": out}

    def snapshot(self, chains, first, count):
        chains = np.asarray(chains, dtype=np.int32)
        n = len(chains)
        state, samples, values = np.empty((n, 4)), np.empty((n, count, self.P)), np.empty((n, count))
        self._ok(self.lib.sepaihrd_mh_snapshot_begin(self.mh, chains.ctypes.data, n, first, count))
        with_values = count > 0 and self.device_streams  # the samples' values are kept with the scale, on the device
        self._ok(self.lib.sepaihrd_mh_snapshot_end(self.mh, 1, state.ctypes.data, samples.ctypes.data if count else None,
                                                   values.ctypes.data if with_values else None))
        out = {"state": state, "samples": samples}
        if with_values:
            out["values"] = values
        return out

    def final(self):
        lib, mh = self.lib, self.mh
        ns = lib.sepaihrd_mh_sample_count(mh)
        out = {"samples": np.empty((CHAINS, ns, self.P)), "best": np.empty((CHAINS, self.P)), "lp": np.empty(CHAINS),
               "best_lp": np.empty(CHAINS), "accepted": np.empty(CHAINS, dtype=np.int32), "cov": np.empty((CHAINS, self.P, self.P))}
        self._ok(lib.sepaihrd_mh_read_samples(mh, 0, ns, out["samples"].ctypes.data))
        self._ok(lib.sepaihrd_mh_read_best(mh, out["best"].ctypes.data))
        self._ok(lib.sepaihrd_mh_read_run_state(mh, out["lp"].ctypes.data, out["best_lp"].ctypes.data, None, out["accepted"].ctypes.data, None))
        self._ok(lib.sepaihrd_mh_read_covariance(mh, out["cov"].ctypes.data))
        return out

    def close(self):
        self.lib.sepaihrd_mh_destroy(self.mh)  # the sampler before its context
        self.mh = None
        self.hip.close()


def _start(mm, synth400):
    pb = synth400.with_(arith=mm.ARITH_FMA, constraint_mode=mm.CONSTRAINT_REFLECT)
    x0 = mm.draws.jitter_draws(pb, 3, CHAINS)
    cov0 = np.diag((0.02 * np.maximum(np.abs(pb.base_theta), 1e-3)) ** 2) + 1e-6 * np.eye(pb.n_params)
    return pb, x0, cov0


def test_sampler_buffers_grow_and_are_reused(mm, synth400):
    """The snapshot's device and page-locked buffers and its chain list (1 chain without samples, 3 chains with 2 samples each,
    1 chain with 1 sample), the rank-one queue's buffers (flushed by the covariance refreshes and the last read) and the lazily
    created events and snapshot stream, between history reads of 1, 3 and 8 rows: every read of ONE sampler equals the same read
    of a fresh sampler stepped to the same iteration, which has made no other read."""
    pb, x0, cov0 = _start(mm, synth400)
    reads = [(3, lambda s: s.history([0])),
             (5, lambda s: s.snapshot([2], 0, 0)),
             (8, lambda s: s.history([1, 4, 7])),
             (11, lambda s: s.snapshot([0, 1, 3], 2, 2)),
             (15, lambda s: s.history([0, 2, 5, 9, 12, 13, 14, 15])),
             (19, lambda s: s.snapshot([1], 6, 1)),
             (ITERS - 1, lambda s: s.final())]
    shared = _Sampler(mm, pb, x0, cov0)
    for i, (done, read) in enumerate(reads):
        fresh = _Sampler(mm, pb, x0, cov0)
        shared.advance(done)
        fresh.advance(done)
        got, want = read(shared), read(fresh)
        _same(got, want, i)
        fresh.close()
    assert 0 < got["accepted"].sum() < CHAINS * (ITERS - 1) and not np.array_equal(got["samples"][:, 0], got["samples"][:, -1])
    shared.close()


def test_create_and_destroy_in_turn(mm, synth400):
    """Ten rounds of a context with a sampler on it (a few iterations each, the sampler destroyed before its context), then a
    context destroyed while no sampler exists: the last round's numbers are the first's."""
    pb, x0, cov0 = _start(mm, synth400)
    rounds = []
    for _ in range(10):
        s = _Sampler(mm, pb, x0, cov0)
        s.advance(7)
        rounds.append({**s.history([0, 3, 7]), **s.snapshot([0, 2], 0, 1)})
        s.close()
    hip = mm.HipObjective(pb)
    alone = hip.eval_batch(x0)
    hip.close()
    _same(rounds[-1], rounds[0], "last round against the first")
    hip = mm.HipObjective(pb)
    _same(hip.eval_batch(x0), alone, "a context after all of it")
    hip.close()
