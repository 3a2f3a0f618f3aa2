"""The Philox draws of the option restatements (wind_ref, waypoint_ref,
airframe_ref): the counter layout of a draw keyed by episode and global env
id, through oracle.cref.philox_np, and the [-1, 1) f32 of a word."""
import numpy as np

from oracle import cref


def blocks(seed, gids, ep, word):
    """The Philox blocks of counters (ep, gid_lo, gid_hi, word) under key
    `seed`; gids / ep / word scalars or (n,) arrays.  Returns (n,4) uint32."""
    gids = np.atleast_1d(np.asarray(gids)).astype(np.uint64)
    n = len(gids)
    m32 = np.uint64(0xffffffff)
    ep = np.broadcast_to(np.asarray(ep).astype(np.int64).astype(np.uint64) & m32, (n,))
    word = np.broadcast_to(np.asarray(word).astype(np.int64).astype(np.uint64) & m32, (n,))
    ctr = np.stack([ep, gids & m32, gids >> np.uint64(32), word], 1)
    return cref.philox_np(ctr, [seed & 0xffffffff, (seed >> 32) & 0xffffffff])


def pm1(words):
    """f32(2u - 1) of the words' uniforms u = w * 2^-32 (exact in f64, then
    the one rounding)."""
    return (2.0 * (words.astype(np.float64) * 2.0 ** -32) - 1.0).astype(np.float32)
