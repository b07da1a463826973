"""The problems and option blocks away from their defaults that tests/test_off_defaults_cpu.py (conditions, no GPU),
tests/test_gpu_step.py and tests/test_gpu_off_defaults.py share: a y pixel pitch that differs from the x pitch, scale 1 and 3, other
loss scales, LM-diagonal clamps that bind and loop options that end or bend the trajectory.  The tuples behind the loop options are
(iterations, accepted, rejected, termination) of oracle.solve on BASE, recorded from the CPU oracle."""
import dataclasses

import numpy as np

from lifcal_amd import _capi as capi
from tests.helpers import S

A = 1.25                                                    # spy = A spx
BASE = S(6, 40, None, 0x506, 101)
ROBUST = S(6, 40, None, 0xF06, 102, outlier_fraction=0.05)
SCALE_1 = dataclasses.replace(BASE, scale=1)                # 1141 observations
SCALE_3 = dataclasses.replace(BASE, scale=3)                # 1145 observations
RADIUS = 1e4

TERM_FUNCTION, TERM_GRADIENT, TERM_MAX_ITERATIONS, TERM_MIN_RADIUS = 1, 3, 4, 5

# name -> (options, sides of the clamp the case is there for); clip counts on BASE at RADIUS, of 165 live entries, (below, above):
CLAMPS = {
    "lm_min_binds": (dict(min_lm_diagonal=0.9), ("below",)),                                                            # (138, 0)
    "lm_max_binds": (dict(max_lm_diagonal=0.5), ("above",)),                                                            # (0, 87)
    "lm_both_bind_unscaled": (dict(jacobi_scaling=0, min_lm_diagonal=1e2, max_lm_diagonal=1e6), ("below", "above")),    # (138, 23)
}
LOSS_SCALES = {"loss_scale_02": 0.2, "loss_scale_3": 3.0}  # on ROBUST: 24 and 41 iterations (0.5: 26)

# name -> options; the oracle's (iterations, accepted, rejected, termination) on BASE
LOOP = {
    "defaults": dict(),                                                             # 13, 12, 0, 1
    "gradient_tolerance_at_the_first_sweep": dict(gradient_tolerance=1e30),         # 0, 0, 0, 3
    "gradient_tolerance_after_steps": dict(gradient_tolerance=1e3),                 # 3, 3, 0, 3
    "min_radius_at_once": dict(initial_radius=1e-30, min_radius=1e-20),             # 0, 0, 0, 5
    "max_radius_caps": dict(max_radius=3e4, max_iterations=30),                     # 30, 30, 0, 4, final radius 3e4
    "initial_radius_small": dict(initial_radius=1e-2),                              # 27, 26, 0, 1
    "min_relative_decrease_rejects": dict(min_relative_decrease=0.9),               # 21, 14, 6, 1
    "lm_min_2": dict(min_lm_diagonal=2.0),                                          # 14, 13, 0, 1
    "lm_max_05": dict(max_lm_diagonal=0.5),                                         # 14, 12, 1, 1
    "lm_1e2_1e6_unscaled": dict(jacobi_scaling=0, min_lm_diagonal=1e2, max_lm_diagonal=1e6),     # 12, 11, 0, 1
}
UNTOUCHED = ("gradient_tolerance_at_the_first_sweep", "min_radius_at_once")   # no step is taken: the parameters come back as they went in


def options(**kw):
    o = capi.default_options_py()
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


def clip_counts(ne, lm_min, lm_max):
    """(below, above): the live entries of h sigma^2 the LM-diagonal clamp moves, by tests/step_reference.NormalEquations' own h, sigma"""
    t = (ne.h.astype(np.float64) * ne.sigma * ne.sigma)[ne.live]
    return int(np.sum(t < lm_min)), int(np.sum(t > lm_max))


def tuple_of(s):
    return (int(s.iterations), int(s.successful_steps), int(s.unsuccessful_steps), int(s.termination))
