"""Shape tables and seeded instance generators that more than one test module (and tools/) use."""
import numpy as np


# (N, nx, nu, nc) -> the kernel fbstab_hip_mpc_create must pick (fbstab_hip.hip:
# record_instance_for); four shapes per instance, exact and padded.
MPC_SHAPES = [
    ((6, 12, 4, 20), "fbstab_mpc_r16_kernel<12,4,20>"), ((9, 5, 2, 7), "fbstab_mpc_r16_kernel<12,4,20>"),
    ((3, 12, 1, 17), "fbstab_mpc_r16_kernel<12,4,20>"), ((11, 1, 4, 1), "fbstab_mpc_r16_kernel<12,4,20>"),
    ((5, 12, 4, 32), "fbstab_mpc_r16_kernel<12,4,32>"), ((8, 7, 3, 21), "fbstab_mpc_r16_kernel<12,4,32>"),
    ((2, 11, 4, 27), "fbstab_mpc_r16_kernel<12,4,32>"), ((12, 3, 1, 30), "fbstab_mpc_r16_kernel<12,4,32>"),
    ((7, 18, 5, 10), "fbstab_mpc_r32_kernel<18,5,10>"), ((4, 13, 2, 6), "fbstab_mpc_r32_kernel<18,5,10>"),
    ((10, 16, 5, 9), "fbstab_mpc_r32_kernel<18,5,10>"), ((3, 12, 5, 3), "fbstab_mpc_r32_kernel<18,5,10>"),
    ((5, 24, 8, 16), "fbstab_mpc_r32_kernel<24,8,16>"), ((6, 20, 6, 16), "fbstab_mpc_r32_kernel<24,8,16>"),
    ((9, 19, 2, 12), "fbstab_mpc_r32_kernel<24,8,16>"), ((2, 14, 7, 11), "fbstab_mpc_r32_kernel<24,8,16>"),
    ((4, 24, 8, 32), "fbstab_mpc_r32_kernel<24,8,32>"), ((7, 20, 6, 30), "fbstab_mpc_r32_kernel<24,8,32>"),
    ((3, 22, 3, 17), "fbstab_mpc_r32_kernel<24,8,32>"), ((8, 13, 8, 25), "fbstab_mpc_r32_kernel<24,8,32>"),
    ((4, 26, 3, 9), "fbstab_mpc_kernel<64>"), ((3, 10, 9, 12), "fbstab_mpc_kernel<64>"),
    ((5, 8, 2, 33), "fbstab_mpc_kernel<64>"), ((2, 25, 9, 5), "fbstab_mpc_kernel<64>"),
]


# The degenerate dense family.
# tools/fuzz_dense.py 200 <seed> 64: random shapes with up to 239 inequality rows over at
# most 64 variables.  The shapes below are the ones on which the NATURAL elimination order
# of the one-wavefront kernel took a different number of proximal or Newton iterations than
# the oracle (seed 11: the seven shapes of profiles/r03_af_dense_factorisation_orders.txt;
# seeds 12 and 13: profiles/r04_a_dense_order_choice.txt); the instances are regenerated from
# the tool's own random stream.
DEGENERATE_SHAPES = {11: [(38, 20, 172), (46, 16, 205), (52, 11, 226), (36, 6, 196), (41, 22, 200), (31, 15, 106),
                          (25, 5, 170)],
                     12: [(30, 2, 130), (35, 17, 144), (31, 12, 170), (41, 19, 179), (40, 20, 152), (34, 3, 205),
                          (42, 17, 137)],
                     13: [(38, 20, 109), (41, 22, 87), (45, 19, 167), (51, 12, 234), (43, 6, 231), (35, 17, 168),
                          (33, 14, 232), (34, 15, 171)]}


def fuzz_dense_instances(seed, wanted, n=200, kmax=64):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        nz = int(rng.integers(1, 160)); nl = int(rng.integers(0, min(nz, 24) + 1)); nv = int(rng.integers(1, 240))
        nz = int(rng.integers(1, kmax + 1)); nl = int(rng.integers(0, min(nz, 24, kmax - nz) + 1))
        B = int(rng.integers(1, 10))
        first_id = int(rng.integers(0, 1 << 20))
        if (nz, nl, nv) in wanted:
            out.append((nz, nl, nv, B, first_id))
    return out


# (nz, nl, nv), threads per QP, what DenseLayout::init must say (k_global, v_global), spread: one shape per dense
# kernel - the one-wavefront kernel (twice, and once without equalities), four wavefronts with K in LDS, K in
# global scratch, and the smallest nv at (20, 5) that moves the iterate vectors to global scratch too
DENSE_KERNEL_SHAPES = [
    ((50, 10, 100), 64, (0, 0), 1.09e-6), ((60, 4, 131), 64, (0, 0), 1.15e-6), ((30, 0, 40), 64, (0, 0), 6.06e-7),
    ((90, 12, 77), 256, (0, 0), 1.62e-6), ((159, 24, 239), 256, (1, 0), 4.44e-6),
    ((20, 5, 2534), 256, (1, 1), 2.59e-7),
]
# The generator makes a quarter of the rows active: at (20, 5, 2534) that is 630 active rows on 20 variables, a
# degenerate vertex at which the multipliers are not unique and V is singular but for sigma.  There the
# reference's own two roundings part by more than the residual rule allows (Oracle(fma=True) leaves 4.5 x the
# residual of Oracle() on QP 2 of these three, and their steps differ by 1.6e-3), so the rule has nothing to
# compare against.  The v_global shape therefore relaxes every row from RELAX_FROM on by RELAX (they become
# inactive; 15 rows stay active): same kernel, same vector lengths, a QP with a unique answer.
RELAX_FROM, RELAX = 40, 10.0
