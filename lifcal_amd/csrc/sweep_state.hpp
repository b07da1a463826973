// sweep_state.hpp — what the host knows about the two things a sweep used to rebuild in front of itself, written once:
//   1  the table sets (camera constants | frame table | lens table): the CURRENT set (Dev::camc, ft, lt, and ltf, ltw with
//      options.precision = 1) and the CANDIDATE set (Dev::camc_c, ft_c, lt_c).  A set is a pure function of the parameter arrays
//      it was built from and of the two build flags (tangents, fold), so a sweep builds the current set only when the record says
//      that it is not the set of the current parameters, with tangents, folded.
//   2  the two copies of the reduced block (Sband | Sarrow | rhsacc | gB | hdiag | scal | step scalars): a sweep accumulates into
//      the copy the previous sweep did not use; the previous sweep's k_finalize has zero-filled it.  A copy that is not known to be
//      zero gets an explicit fill first.
// Every writer of a table set or of a parameter array reports here; no call site reasons about reuse on its own.
// Parameter contents are named by generation numbers: a write makes a new one, a pointer swap moves them, a copy copies them.
// Nothing from HIP in here: the header also compiles as plain C++ (tests/test_sweep_state_cpu.py drives it through a C shim).
#pragma once
#include <stdint.h>

namespace lifcal {

enum { SS_CURRENT = 0, SS_CANDIDATE = 1 };

struct SsTables { uint32_t src; bool tangents, fold; };   // src: generation of the parameters the set was built from, 0 = not usable

struct SweepState {
  uint32_t next_gen;
  uint32_t par[2];      // generation held by the current / candidate parameter arrays (cam | views; points enter no table)
  SsTables tab[2];      // the current / candidate table set
  int bound;            // the copy of the reduced block Dev points at
  bool clean[2];        // copy is known to be all zero (block and step scalars)
};

inline void ss_reset(SweepState* s) {
  s->next_gen = 1; s->par[0] = s->par[1] = 0;
  s->tab[0] = s->tab[1] = SsTables{0, false, false};
  s->bound = 0; s->clean[0] = s->clean[1] = false;
}

// ---- parameters ----------------------------------------------------------------------------------------------------------------
// upload_parameters: new current parameters, the candidate arrays are a copy of them
inline void ss_upload(SweepState* s) { s->par[SS_CURRENT] = s->par[SS_CANDIDATE] = s->next_gen++; }
// k_update_reduced / k_backsub / k_apply_step: a new candidate point
inline void ss_candidate_written(SweepState* s) { s->par[SS_CANDIDATE] = s->next_gen++; }
// swap_current_candidate: the parameter POINTERS change places (the table sets stay where they are)
inline void ss_swap_parameters(SweepState* s) { const uint32_t t = s->par[0]; s->par[0] = s->par[1]; s->par[1] = t; }

// ---- tables --------------------------------------------------------------------------------------------------------------------
inline bool ss_tables_ok(const SweepState* s, int set) {
  const SsTables& t = s->tab[set];
  return t.src != 0 && t.src == s->par[set] && t.tangents && t.fold;
}
// what launch_sweep and the trial sweeps of the line search ask
inline bool ss_sweep_needs_tables(const SweepState* s) { return !ss_tables_ok(s, SS_CURRENT); }
// launch_tables wrote table set `set` from parameter arrays `from`
inline void ss_tables_built(SweepState* s, int set, int from, bool tangents, bool fold) { s->tab[set] = SsTables{s->par[from], tangents, fold}; }
// somebody used the arrays of a set for something else
inline void ss_tables_clobbered(SweepState* s, int set) { s->tab[set].src = 0; }

// host loop, accepted step: the parameter pointers change places, and with them (with_tables) the table pointers.  Without the
// table swap (options.precision = 1: the fp32 lens table has no candidate twin) the current set keeps the generation of the point
// just left, so the next sweep finds it stale by the comparison above and rebuilds it once.
inline void ss_host_accept(SweepState* s, bool with_tables) {
  ss_swap_parameters(s);
  if (with_tables) { const SsTables t = s->tab[0]; s->tab[0] = s->tab[1]; s->tab[1] = t; }
}
// device loop, k_lm_commit: the kernel copies candidate parameters AND candidate tables over the current ones if the step was
// accepted, and nothing otherwise — the host does not know which.  Either way the current set belongs to the current parameters
// afterwards, provided both sets were right before.
inline void ss_device_commit(SweepState* s) {
  const bool ok = ss_tables_ok(s, SS_CURRENT) && ss_tables_ok(s, SS_CANDIDATE);
  s->par[SS_CURRENT] = s->next_gen++;
  s->tab[SS_CURRENT] = ok ? SsTables{s->par[SS_CURRENT], true, true} : SsTables{0, false, false};
}

// ---- the two copies of the reduced block ---------------------------------------------------------------------------------------
// a kernel chain is about to accumulate: switch to the other copy.  true: it is not known to be zero, fill it first
inline bool ss_acquire_block(SweepState* s) {
  s->bound ^= 1;
  const bool fill = !s->clean[s->bound];
  s->clean[s->bound] = false;
  return fill;
}
// k_finalize of the sweep that filled the bound copy has zero-filled the other one
inline void ss_finalize_cleaned_other(SweepState* s) { s->clean[s->bound ^ 1] = true; }

}  // namespace lifcal
