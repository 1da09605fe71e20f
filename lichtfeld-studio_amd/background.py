"""Background colour policy of the trainer: which colour a training step composites its render - and an RGBA target - over. Pure host functions, no
device tensor and no device read: the fastgs route hands the three floats to its kernels by value.

  constant   the base colour on every step ("black", "white" or a triple in [0,1]; the official trainer's --white_background)
  random     one colour per STEP from a CPU generator (the official trainer's random_background): transparent is then the only consistent explanation of a pixel
             whose target alpha is 0
  modulated  the reference's OptimizationParameters::bg_modulation (trainer.cpp:474-577): a sine-modulated colour mixed into the base colour with a weight that
             holds 1 for the first quarter of the run, falls to 0.5 at the half and to 0 at three quarters; from there on the base colour alone

The reference draws the modulation's jitter on the device (torch::rand on kCUDA): its colours differ from run to run and cost a device generator call per step. Here the
jitter comes from the same seeded CPU generator as the random mode - identical on every rank and in every rerun. That difference is deliberate."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np

MODES = ("constant", "random", "modulated")
NAMED = {"black": (0.0, 0.0, 0.0), "white": (1.0, 1.0, 1.0)}
PERIODS = (37, 41, 43)
JITTER_AMPLITUDE = 0.03      # the jitter is (u - 0.5) * 0.06, u uniform in [0,1)
CLAMP = 1e-4


def parse_background(background) -> Tuple[float, float, float]:
    """"black" | "white" | three numbers -> the triple; every component finite and in [0,1]"""
    if isinstance(background, str):
        if background not in NAMED:
            raise ValueError(f"background must be 'black', 'white' or three numbers in [0,1] (got {background!r})")
        return NAMED[background]
    try:
        bg = tuple(float(v) for v in background)
    except TypeError:
        raise ValueError(f"background must be 'black', 'white' or three numbers in [0,1] (got {background!r})") from None
    if len(bg) != 3 or not all(math.isfinite(v) and 0.0 <= v <= 1.0 for v in bg):
        raise ValueError(f"background must be three finite numbers in [0,1] (got {background!r})")
    return bg


def inv_weight_piecewise(step: int, max_steps: int) -> float:
    """the mix weight of the modulated colour at `step` of `max_steps`, in float32: 1 while step / max_steps < 1/4, linear to 0.5 at 1/2, linear to 0 at 3/4 and
    NEGATIVE beyond (the line is not clamped: background_for_step tests w <= 0, as the reference does)"""
    f = np.float32
    phase = max(f(0), min(f(1), f(step) / f(max(1, max_steps))))
    if phase < f(0.25):
        return 1.0
    if phase < f(0.5):
        t = (phase - f(0.25)) / (f(0.5) - f(0.25))
        return float(f(1) + (f(0.5) - f(1)) * t)
    t = (phase - f(0.5)) / (f(0.75) - f(0.5))
    return float(f(0.5) + (f(0) - f(0.5)) * t)


def sine_background(step: int, jitter: Optional[np.ndarray] = None) -> np.ndarray:
    """0.5 (1 + sin(2 pi (step mod P_c) / P_c + 2 pi c / 3)) for the periods 37 / 41 / 43, plus `jitter` (three float32 values or None), clamped to
    [1e-4, 1 - 1e-4]; float32 arithmetic"""
    f = np.float32
    two_pi = f(2.0 * math.pi)
    out = np.empty(3, f)
    for c, period in enumerate(PERIODS):
        phase = two_pi * (f(step % period) / f(period))
        out[c] = f(0.5) * (f(1) + np.sin(phase + f(c) * two_pi / f(3), dtype=f))
    if jitter is not None:
        out = out + np.asarray(jitter, f)
    return np.clip(out, f(CLAMP), f(1) - f(CLAMP)).astype(f)


def _rand3(generator) -> np.ndarray:
    import torch
    if generator is None or generator.device.type != "cpu":
        raise ValueError("the background colours are drawn from a CPU torch.Generator (the same on every rank, no device read)")
    return torch.rand(3, generator=generator, dtype=torch.float32).numpy()


def background_for_step(iteration: int, iterations: int, base=(0.0, 0.0, 0.0), mode: str = "constant", generator=None, jitter: bool = True) -> Tuple[float, float, float]:
    """The colour of (1-based) `iteration` of a run of `iterations` -> three Python floats.
    constant: base. random: torch.rand(3) from `generator` (a CPU generator; one draw per call - call it once per step). modulated: with
    w = inv_weight_piecewise(iteration, iterations), base when w <= 0 (from 3/4 of the run on), else (1 - w) base + w sine_background(iteration), the jitter
    (rand(3) - 0.5) * 0.06 drawn from `generator` when `jitter` is on (no draw once w <= 0)."""
    if mode not in MODES:
        raise ValueError(f"background_mode must be one of {MODES} (got {mode!r})")
    base = parse_background(base)
    if mode == "constant":
        return base
    if mode == "random":
        return tuple(float(v) for v in _rand3(generator))
    f = np.float32
    w = f(inv_weight_piecewise(int(iteration), int(iterations)))
    if w <= 0:
        return base
    jit = (_rand3(generator) - f(0.5)) * f(2.0 * JITTER_AMPLITUDE) if jitter else None
    sine = sine_background(int(iteration), jit)
    mixed = np.asarray(base, f) * (f(1) - w) + w * sine
    return tuple(float(v) for v in mixed)
