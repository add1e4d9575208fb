"""The order of csrc/nslam_reduce.h's float64 sums in numpy float64 (no GPU): what a workgroup's threads hold goes in,
the bits the device stores come out.  The build has -ffp-contract=off, so a product or a sum rounds here as it does
there, and a test that forms the per-thread values as the kernel writes them can compare int64 bit patterns.

    wave_tree(v)     64 lanes -> lane 0 of the tree with offsets 32, 16, .. 1
    group_sum(t)     256 threads -> the tree per wave, then wave 0's value + wave 1's + wave 2's + wave 3's
    ordered_sum(p)   partials in index order: one sequential chain that starts at +0
"""
import numpy as np

WAVE = 64
THREADS = 256


def wave_tree(v):
    """v [..., 64] -> [...]: at offset d lane l < d takes v[l] + v[l + d]; lane 0 after d = 32, 16, .. 1."""
    v = np.asarray(v, dtype=np.float64)
    assert v.shape[-1] == WAVE
    d = WAVE // 2
    while d >= 1:
        v = v[..., :d] + v[..., d:2 * d]
        d //= 2
    return v[..., 0]


def group_sum(t):
    """t [..., 256] (thread order) -> [...]: the workgroup's total."""
    t = np.asarray(t, dtype=np.float64)
    assert t.shape[-1] == THREADS
    w = wave_tree(t.reshape(t.shape[:-1] + (THREADS // WAVE, WAVE)))
    s = w[..., 0]
    for k in range(1, THREADS // WAVE):
        s = s + w[..., k]
    return s


def ordered_sum(p):
    """p [n, ...] -> [...]: ((+0 + p[0]) + p[1]) + ... ."""
    p = np.asarray(p, dtype=np.float64)
    s = np.zeros(p.shape[1:])
    for row in p:
        s = s + row
    return s


def thread_sum(terms):
    """terms [rounds, ...] -> [...]: a thread's accumulator after adding its terms in ascending order from +0.  A
    term of +0 stands for a skipped one: it leaves an accumulator that started at +0 as it is."""
    return ordered_sum(terms)


def bits(a):
    """The int64 bit patterns of a float64 array (what the tests compare)."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
