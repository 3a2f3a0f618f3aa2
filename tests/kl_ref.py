"""NumPy restatement of the KL gate of the optimizer step (DESIGN.md section
22): what the Adam-apply launch of step j decides from slot j of the control
block and the step's approx_kl, and what it leaves in slot j + 1.  SB3 is not
installed; this text is the contract the kernels are held to.

A slot is (stopped, taken, lr): whether the iteration has stopped, how many
steps it has applied, the learning rate (f32).  In this order:

  1. stopped: nothing is applied, the next slot is a copy;
  2. target_kl set and kl > f32(1.5 * target_kl) (false for NaN): stopped <- 1,
     taken and lr carried, nothing applied -- the tripping minibatch is not;
  3. adaptive, in f32 with one rounding per operation:
       kl > 2 desired_kl        lr <- max(lr / 1.5, lr_min)
       0 < kl < desired_kl / 2  lr <- min(lr * 1.5, lr_max)
  4. the step is applied with the Adam scalars of row `taken` of the
     iteration's table (not row j: a skipped step does not advance Adam's step
     count); step_size = table[taken][0], or adaptive (a table built at lr 1)
     f32(lr * table[taken][0]); the next slot is (0, taken + 1, lr).
"""
from typing import NamedTuple

import numpy as np

f32 = np.float32


class Slot(NamedTuple):
    stopped: int
    taken: int
    lr: np.float32

    def words(self):
        """The slot's four device words."""
        return np.array([self.stopped, self.taken, f32(self.lr).view(np.uint32), 0], np.uint32)


def stop_kl(target_kl):
    """f32(1.5 * target_kl): the product in double, one rounding."""
    return None if target_kl is None else f32(1.5 * target_kl)


def gate(slot, kl, target_kl=None, adaptive=False, desired_kl=0.01, lr_min=1e-6, lr_max=1e-2):
    """One step's decision.  Returns (next slot, applied) with applied None
    for a skipped step, else (table row, lr used)."""
    kl = f32(kl)
    if slot.stopped:
        return slot, None
    if target_kl is not None and kl > stop_kl(target_kl):
        return Slot(1, slot.taken, slot.lr), None
    lr = f32(slot.lr)
    if adaptive:
        high, low = f32(2 * desired_kl), f32(desired_kl / 2)
        if kl > high:
            lr = max(f32(lr / f32(1.5)), f32(lr_min))
        elif f32(0) < kl < low:
            lr = min(f32(lr * f32(1.5)), f32(lr_max))
    return Slot(0, slot.taken + 1, lr), (slot.taken, lr)


def step_scalars(table, applied, adaptive=False):
    """(step_size, sqrt(bias_correction2)) of an applied step from the
    iteration's (S, 2) f32 table."""
    row, lr = applied
    s0, s1 = f32(table[row][0]), f32(table[row][1])
    return (f32(lr * s0) if adaptive else s0), s1


def run(kls, lr0, **settings):
    """The gate over an iteration's approx_kl sequence from slot 0 =
    (0, 0, lr0).  Returns (slots: S + 1, applied: S entries, None = skipped)."""
    slots, applied = [Slot(0, 0, f32(lr0))], []
    for kl in kls:
        nxt, ap = gate(slots[-1], kl, **settings)
        slots.append(nxt)
        applied.append(ap)
    return slots, applied


def adam_table(lr, b1, b2, first_step, count):
    """torch.optim.Adam's step-dependent scalars for steps first_step ..
    first_step + count - 1: (lr / (1 - b1^t), sqrt(1 - b2^t)) formed in double,
    then f32."""
    t = np.arange(first_step, first_step + count, dtype=np.float64)
    return np.stack([lr / (1.0 - b1 ** t), np.sqrt(1.0 - b2 ** t)], axis=1).astype(f32)


def clip_adam(p, g, m, v, step_size, bc2_sqrt, b1=0.9, b2=0.999, eps=1e-5, max_norm=0.5):
    """clip_grad_norm_ + Adam in f32 on copies (the CPU stand-in for the
    kernel's arithmetic; the GPU tests use the ungated kernel instead).
    Returns (p, g, m, v)."""
    p, g, m, v = (np.array(x, f32) for x in (p, g, m, v))
    total = f32(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    c = min(f32(max_norm) / (total + f32(1e-6)), f32(1.0))
    g = g * c
    m = m + f32(1.0 - b1) * (g - m)
    v = v * f32(b2) + (f32(1.0 - b2) * g) * g
    p = p + (-f32(step_size)) * (m / (np.sqrt(v) / f32(bc2_sqrt) + f32(eps)))
    return p, g, m, v


def run_adam(kls, grads, p, m, v, table, lr0, apply=clip_adam, **settings):
    """The gate over (kl, grads) pairs with `apply` as the step.  Returns
    (slots, applied, states) with states[j] = (p, m, v) after step j."""
    slots, applied = run(kls, lr0, **settings)
    states = []
    for ap, g in zip(applied, grads):
        if ap is not None:
            s0, s1 = step_scalars(table, ap, settings.get("adaptive", False))
            p, _, m, v = apply(p, g, m, v, s0, s1)
        states.append((p, m, v))
    return slots, applied, states
