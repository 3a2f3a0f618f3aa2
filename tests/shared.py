"""Helpers that several test files defined word for word."""
import numpy as np


def gym_state(g):
    """The oracle's state dict from a golden file's arrays; copies, because
    the oracle steps its state in place."""
    s = {k: np.array(g[k], np.float64, order="C")
         for k in ("pos", "vel", "euler", "omega", "target")}
    s["step"] = np.array(g["step"], np.int32)
    return s


def bits(a):
    """A NumPy array's words as unsigned integers, for bitwise comparison."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def gym_batch(n, **kw):
    from drone_rl_amd import DroneBatch
    return DroneBatch(n, "gym", **kw)


def f32_bits(t):
    """An f32 tensor's words."""
    return t.cpu().numpy().view(np.uint32)
