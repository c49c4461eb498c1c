"""The host's placement rules for a precedence model's fused launch (csrc/sf_mixed_plan.h: plan_generic_launch), restated once for the GPU tests
that assert the placement the library recorded (test_gpu_prec_placement.py, test_gpu_precedence.py, test_gpu_precedence_leaf.py).
n nodes, E valid fixed edges, V lists; all integer.  test_generic_plan.py checks this restatement against the library.  Not a test module."""


def a16(x):
    return (x + 15) // 16 * 16


def pgrp_bytes(n, t, V):
    """sf_prec_group.h: pgrp_bytes -- the grouped evaluator's scratch for t trials per wavefront."""
    if t <= 0:
        return 0
    a2 = a16(2 * n)
    return 4 * a2 + a16(4 * V) + t * (2 * a16(4 * (n + 64 // t)) + 2 * a2)


def default_trials(n, V):
    """The default rule for the grouped evaluator (full static copy present): g = largest power of two <= max(V, 2), t = min(16, 64 / g),
    halved until the scratch is at most 14 KiB or scratch + 16 n + 2,560 at most 20 KiB; 0 = off."""
    g = 1
    while g * 2 <= max(V, 2):
        g *= 2
    t = min(16, 64 // g)
    while t >= 2:
        b = pgrp_bytes(n, t, V)
        if b <= 14 * 1024 or b + 16 * n + 2560 <= 20 * 1024:
            return t
        t >>= 1
    return 0


def forced_trials(n, V, t):
    """SF_AMD_PREC_GROUPS=t (2 / 4 / 8 / 16, anything else 0): halved while the scratch passes 40 KiB."""
    if t not in (2, 4, 8, 16):
        return 0
    while t > 1 and pgrp_bytes(n, t, V) > 40 * 1024:
        t >>= 1
    return t if t > 1 else 0


def static_copy(n, E, owner, slim=True):
    """The workgroup-shared copy of the static graph by its byte rules alone (Kahn scratch in LDS, room beside the slice):
    1 full (<= 16 KiB), 2 slim (<= 40 KiB), 0 none."""
    if (28 if owner else 24) * n + 8 * E + 24 <= 16 * 1024:
        return 1
    return 2 if slim and (16 if owner else 12) * n + 16 <= 40 * 1024 else 0


def trials(n, V, static, forced=None):
    """T of a launch with the Kahn scratch in LDS: the grouped evaluator needs the full copy; forced = the value of SF_AMD_PREC_GROUPS."""
    if static != 1:
        return 0
    return default_trials(n, V) if forced is None else forced_trials(n, V, forced)
