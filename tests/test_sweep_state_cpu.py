"""The host-side record of lifcal_amd/csrc/sweep_state.hpp (which parameters each table set was built from; which copy of the reduced
block is known to be zero), compiled as plain C++ (no HIP) behind a C shim.

The driver below does what lifcal_ba.hip does with the record, call for call, and keeps a model of the device memory of its own: the
CONTENT of the two parameter arrays (an integer per distinct point), the content of the two table sets (parameter content, tangents,
fold) and whether each copy of the block is zero.  The model never looks into the record; the record never sees the model.  After
every event two invariants are checked where they bite, inside the sweep:
  * a sweep never runs on tables whose source parameters differ from the current ones (or that lack tangents / folding);
  * a sweep never accumulates into a copy of the block that is not zero.
"""
import ctypes as C
import itertools
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r"""
#include "sweep_state.hpp"
using namespace lifcal;
extern "C" {
int shim_sizeof() { return (int)sizeof(SweepState); }
void shim_reset(SweepState* s) { ss_reset(s); }
void shim_upload(SweepState* s) { ss_upload(s); }
void shim_candidate_written(SweepState* s) { ss_candidate_written(s); }
void shim_swap_parameters(SweepState* s) { ss_swap_parameters(s); }
int shim_sweep_needs_tables(const SweepState* s) { return ss_sweep_needs_tables(s) ? 1 : 0; }
void shim_tables_built(SweepState* s, int set, int from, int tangents, int fold) { ss_tables_built(s, set, from, tangents != 0, fold != 0); }
void shim_tables_clobbered(SweepState* s, int set) { ss_tables_clobbered(s, set); }
void shim_host_accept(SweepState* s, int with_tables) { ss_host_accept(s, with_tables != 0); }
void shim_device_commit(SweepState* s) { ss_device_commit(s); }
int shim_acquire_block(SweepState* s) { return ss_acquire_block(s) ? 1 : 0; }
void shim_finalize_cleaned_other(SweepState* s) { ss_finalize_cleaned_other(s); }
int shim_bound(const SweepState* s) { return s->bound; }
}
"""

CUR, CAND = 0, 1


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the header must compile without hipcc")
    d = tmp_path_factory.mktemp("sweep_state")
    src, lib = os.path.join(str(d), "shim.cpp"), os.path.join(str(d), "libsweep_state_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lifcal_amd", "csrc"), "-o", lib, src])
    so = C.CDLL(lib)
    for fn in ("shim_reset", "shim_upload", "shim_candidate_written", "shim_swap_parameters", "shim_device_commit", "shim_finalize_cleaned_other"):
        getattr(so, fn).argtypes = [C.c_void_p]; getattr(so, fn).restype = None
    so.shim_sweep_needs_tables.argtypes = [C.c_void_p]
    so.shim_tables_built.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]; so.shim_tables_built.restype = None
    so.shim_tables_clobbered.argtypes = [C.c_void_p, C.c_int]; so.shim_tables_clobbered.restype = None
    so.shim_host_accept.argtypes = [C.c_void_p, C.c_int]; so.shim_host_accept.restype = None
    so.shim_acquire_block.argtypes = [C.c_void_p]
    so.shim_bound.argtypes = [C.c_void_p]
    return so


class Driver:
    """lifcal_ba.hip's use of the record, with a model of what the kernels would do to device memory"""

    def __init__(self, so, precision=0):
        self.so = so
        self.precision = precision
        self.buf = C.create_string_buffer(so.shim_sizeof())
        self.s = C.addressof(self.buf)
        so.shim_reset(self.s)
        self.ids = itertools.count(1)
        # the model: physical arrays behind the (swappable) pointers
        self.par = [None, None]            # content of the arrays d.cam / d.cam_c point at
        self.tab = [None, None]            # content of the sets d.camc.. / d.camc_c.. point at: (parameter content, tangents, fold)
        self.f32 = None                    # parameter content the fp32 lens table (precision 1, no candidate twin) was built from
        self.zero = [False, False]         # copy of the block is all zero
        self.bound = so.shim_bound(self.s)
        self.sigma_valid = False
        self.table_builds = 0              # launches of k_tables for the CURRENT set
        self.fills = 0                     # explicit zero-fills
        self.sweeps = 0
        self.upload()                      # lifcal_ba_create

    # ---- what the launchers do ----
    def _ensure_current_tables(self):
        if self.so.shim_sweep_needs_tables(self.s):
            self.tab[CUR] = (self.par[CUR], True, True)
            self.f32 = self.par[CUR]
            self.table_builds += 1
            self.so.shim_tables_built(self.s, CUR, CUR, 1, 1)

    def _acquire_block(self):
        fill = self.so.shim_acquire_block(self.s)
        self.bound = self.so.shim_bound(self.s)
        if fill:
            self.zero[self.bound] = True
            self.fills += 1

    def _accumulate(self):
        """launch_blocks: the invariants"""
        self._acquire_block()
        assert self.tab[CUR] == (self.par[CUR], True, True), "sweep on tables of another parameter set"
        if self.precision == 1:
            assert self.f32 == self.par[CUR], "sweep on an fp32 lens table of another parameter set"
        assert self.zero[self.bound], "sweep accumulates into a block that is not zero"
        self.zero[self.bound] = False

    def upload(self):
        v = next(self.ids)
        self.par = [v, v]
        self.so.shim_upload(self.s)
        self.sigma_valid = False

    def set_fixed_frames(self):
        self.sigma_valid = False           # (tables do not depend on the frame mask)

    def sweep(self):
        self._ensure_current_tables()
        if not self.sigma_valid:           # the diagonal-only pass
            self._accumulate()
            self.sigma_valid = True
        self._accumulate()
        self.zero[self.bound ^ 1] = True   # k_finalize's extra workgroups
        self.so.shim_finalize_cleaned_other(self.s)
        self.sweeps += 1

    def candidate(self):
        self.par[CAND] = next(self.ids)    # k_update_reduced / k_backsub
        self.so.shim_candidate_written(self.s)
        self._build_candidate_tables()

    def _build_candidate_tables(self):
        self.tab[CAND] = (self.par[CAND], True, True)
        self.so.shim_tables_built(self.s, CAND, CAND, 1, 1)

    def _swap(self):
        self.par.reverse()
        self.so.shim_swap_parameters(self.s)

    def host_accept(self):
        self.par.reverse()
        with_tables = self.precision == 0
        if with_tables:
            self.tab.reverse()
        self.so.shim_host_accept(self.s, 1 if with_tables else 0)

    def device_commit(self, accepted):
        """k_lm_commit: the host does not learn `accepted`"""
        if accepted:
            self.par[CUR] = self.par[CAND]
            self.tab[CUR] = self.tab[CAND]
        self.so.shim_device_commit(self.s)

    def line_search(self, n_trials):
        for _ in range(n_trials):          # eval_trial
            self.par[CAND] = next(self.ids)            # k_apply_step
            self.so.shim_candidate_written(self.s)
            self._swap()
            self._ensure_current_tables()
            self._accumulate()
            self._swap()
        self.par[CAND] = next(self.ids)                # k_apply_step at the chosen step length
        self.so.shim_candidate_written(self.s)
        self._build_candidate_tables()

    def stats(self):
        """calcReprojectionError / projectObservations: unfolded tables of the current point in the candidate arrays"""
        self.tab[CAND] = (self.par[CUR], False, False)
        self.so.shim_tables_clobbered(self.s, CAND)


@pytest.mark.parametrize("precision", [0, 1])
def test_sweeps_on_an_unchanged_point_build_tables_once(shim, precision):
    d = Driver(shim, precision)
    d.sigma_valid = True                   # (no diagonal-only pass: see the next test)
    for _ in range(7):
        d.sweep()
    assert d.table_builds == 1 and d.fills == 1 and d.sweeps == 7


def test_first_sweep_with_the_diagonal_pass(shim):
    """a fresh handle: neither copy is known to be zero, and the first sweep accumulates twice (diagonal-only pass, then the sweep)"""
    d = Driver(shim)
    for _ in range(5):
        d.sweep()
    assert d.table_builds == 1 and d.fills == 2
    d.set_fixed_frames()                   # a new solve on the same parameters: the diagonal pass takes the copy k_finalize cleaned,
    d.sweep()                              # the sweep behind it the one before that, which nobody has cleaned
    assert d.table_builds == 1 and d.fills == 3
    d.sweep()
    assert d.fills == 3


def test_upload_makes_the_tables_stale_even_for_equal_values(shim):
    d = Driver(shim)
    d.sweep(); d.sweep()
    d.upload()
    d.sweep()
    assert d.table_builds == 2
    d.sweep()
    assert d.table_builds == 2


@pytest.mark.parametrize("precision", [0, 1])
def test_stats_calls_between_sweeps(shim, precision):
    d = Driver(shim, precision)
    d.sweep(); d.stats(); d.sweep()
    assert d.table_builds == 1
    # ... and between a candidate and the decision about it: the borrowed candidate arrays must not become current tables
    d.candidate(); d.stats(); d.host_accept(); d.sweep()
    assert d.table_builds == 2
    d.candidate(); d.stats(); d.device_commit(True); d.sweep()
    assert d.table_builds == 3


def test_host_loop_fp64_never_rebuilds_behind_the_first_sweep(shim):
    d = Driver(shim)
    d.sweep()
    for accept in (True, False, False, True, True, False, True):
        d.candidate()
        if accept:
            d.host_accept()
        d.sweep()
    assert d.table_builds == 1 and d.fills == 2


def test_host_loop_precision_1_rebuilds_once_per_accepted_step(shim):
    d = Driver(shim, precision=1)
    d.sweep()
    seq = (True, False, False, True, True, False, True)
    for accept in seq:
        d.candidate()
        if accept:
            d.host_accept()
        d.sweep()
    assert d.table_builds == 1 + sum(seq)


def test_device_loop_never_rebuilds_behind_the_first_sweep(shim):
    d = Driver(shim)
    d.sweep()
    for accept in (True, False, False, True, True, False, True):
        d.candidate()
        d.device_commit(accept)
        d.sweep()                          # the speculative sweep
    assert d.table_builds == 1 and d.fills == 2


@pytest.mark.parametrize("precision", [0, 1])
def test_line_search_trials(shim, precision):
    d = Driver(shim, precision)
    d.sweep()
    builds = d.table_builds
    d.candidate(); d.line_search(3)        # three trial sweeps, each at a new point, into the current set
    assert d.table_builds == builds + 3
    d.sweep()                              # rejected: the current set holds the last trial point
    assert d.table_builds == builds + 4
    d.candidate(); d.line_search(2); d.host_accept(); d.sweep()
    assert d.table_builds == builds + 4 + 2 + (1 if precision == 1 else 0)
    d.candidate(); d.line_search(0); d.host_accept(); d.sweep()   # the Armijo test held at the full step: no trial
    assert d.table_builds == builds + 6 + (2 if precision == 1 else 0)


@pytest.mark.parametrize("seed", range(20))
@pytest.mark.parametrize("precision", [0, 1])
def test_random_event_sequences_keep_the_invariants(shim, seed, precision):
    """the assertions are those inside Driver._accumulate"""
    rng = random.Random(1000 * precision + seed)
    d = Driver(shim, precision)
    have_candidate = False
    for _ in range(400):
        ev = rng.choice(["sweep", "sweep", "candidate", "accept", "reject", "commit", "search", "stats", "upload", "fixed"])
        if ev == "sweep":
            d.sweep()
        elif ev == "candidate":
            d.sweep(); d.candidate(); have_candidate = True
        elif ev == "accept" and have_candidate:
            d.host_accept(); d.sweep(); have_candidate = False
        elif ev == "reject" and have_candidate:
            d.sweep(); have_candidate = False
        elif ev == "commit" and have_candidate and precision == 0:
            d.device_commit(rng.random() < 0.5); d.sweep(); have_candidate = False
        elif ev == "search" and have_candidate:
            d.line_search(rng.randrange(4))
        elif ev == "stats":
            d.stats()
        elif ev == "upload":
            d.upload(); have_candidate = False
        elif ev == "fixed":
            d.set_fixed_frames()
    assert d.sweeps > 50


def test_device_commit_with_a_borrowed_candidate_set_is_not_trusted(shim):
    """not a sequence the driver produces (launch_candidate always precedes k_lm_commit), but the record must not vouch for it"""
    d = Driver(shim)
    d.sweep(); d.candidate(); d.stats()
    d.device_commit(True)
    assert shim.shim_sweep_needs_tables(d.s) == 1
    d.sweep()
