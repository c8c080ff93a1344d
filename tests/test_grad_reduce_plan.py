"""The tile table of the batch-summed gradients (fbstab_amd/csrc/fb_grad_reduce_plan.h, behind
fbstab_hip_*_adjoint_batch_reduced) without a GPU: the header compiles with the host compiler alone, and a driver
that walks the table with plain loops - the kernels' index map, minus the matrix cores - reproduces the gradient
tables of fb_adjoint.h summed over a batch; every entry of every array is covered exactly once; the scratch is
what include/fbstab_hip.h documents; and the new entry points refuse bad arguments before any device call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from fbstab_amd.hip_api import MPC_SEQ, DENSE_ARR
from tests import linear_reference as LR
from tests.hostsim import NO_CONTRACTION
from tests import reduced_helpers as R

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fb_grad_reduce_plan.h"
using namespace fbk;
// usage: walk <file> <batch> dense nz nl nv | walk <file> <batch> mpc N nx nu nc
// file: X then P, each batch x (nz + nl + nv) doubles, a QP's [z l v] contiguous
int main(int argc, char** argv) {
  if (argc < 7) return 1;
  const int B = atoi(argv[2]);
  const bool mpc = argv[3][0] == 'm';
  const GradReducePlan p = mpc ? grad_reduce_plan_mpc(atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]))
                               : grad_reduce_plan_dense(atoi(argv[4]), atoi(argv[5]), atoi(argv[6]));
  const int n = p.nz + p.nl + p.nv;
  const int base[3] = {0, p.nz, p.nz + p.nl};
  std::vector<double> X((size_t)B * n), P((size_t)B * n);
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(X.data(), 8, X.size(), f) != X.size() || fread(P.data(), 8, P.size(), f) != P.size()) return 2;
  fclose(f);
  const int tiles = grad_reduce_tiles(p);
  std::printf("plan %d %d %d %lld %lld\n", tiles, kGradReduceChunk, kGradReduceSlot, grad_reduce_chunks(B),
              grad_reduce_scratch_doubles(p, B));
  int seen = 0;
  for (int g = 0; g < grad_reduce_groups(p); g++) seen += grad_reduce_group_tiles(p, g);
  if (seen != tiles) return 3;
  for (int t = 0; t < tiles; t++) {
    int g, rt, ct;
    grad_reduce_tile(p, t, &g, &rt, &ct);
    for (int m = 0; m < kGradReduceTile; m++) {
      const int r = rt * kGradReduceTile + m;
      if (r >= grad_reduce_group_rows(p, g)) continue;  // (the kernel's lanes outside the edge supply zeros)
      int arr, off;
      grad_reduce_row(p, g, r, &arr, &off);
      const int ro = base[arr] + off;
      if (off < 0 || off >= (arr == 0 ? p.nz : arr == 1 ? p.nl : p.nv)) return 4;
      int seq;
      long long idx;
      double scale;
      for (int nn = 0; nn < kGradReduceTile; nn++) {
        const int c = ct * kGradReduceTile + nn;
        if (!grad_reduce_matrix_entry(p, g, r, c, &seq, &idx, &scale)) continue;
        const int co = grad_reduce_col(p, g, c);
        if (co < 0 || co >= p.nz) return 5;
        double s = 0.0;
        for (int b = 0; b < B; b++)
          s += P[(size_t)b * n + ro] * X[(size_t)b * n + co] + X[(size_t)b * n + ro] * P[(size_t)b * n + co];
        std::printf("e %d %lld %.17g\n", seq, idx, scale * s);
      }
      if (ct == 0 && grad_reduce_vector_entry(p, g, r, &seq, &idx, &scale)) {
        double s = 0.0;
        for (int b = 0; b < B; b++) s += P[(size_t)b * n + ro];
        std::printf("e %d %lld %.17g\n", seq, idx, scale * s);
      }
    }
  }
  return 0;
}
'''

BATCH = 5


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("grad_reduce_plan")
    src = d / "walk.cc"
    src.write_text(DRIVER)
    exe = str(d / "walk")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", NO_CONTRACTION,
                           "-I" + R.CSRC, "-o", exe, str(src)])
    return exe, d


def _walk(driver, kind, shape, lens, names, batch=BATCH, seed=0):
    """(plan line, {name: array walked from the table}, per-entry cover counts, x, step)."""
    exe, d = driver
    if kind == "mpc":
        N, nx, nu, nc = shape
        nz, nl, nv = (N + 1) * (nx + nu), (N + 1) * nx, (N + 1) * nc
    else:
        nz, nl, nv = shape
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((batch, nz + nl + nv))
    P = rng.standard_normal((batch, nz + nl + nv))
    path = d / ("%s_%s.bin" % (kind, "_".join(map(str, shape))))
    with open(path, "wb") as f:
        f.write(X.tobytes())
        f.write(P.tobytes())
    out = subprocess.run([exe, str(path), str(batch), kind] + [str(s) for s in shape], capture_output=True, text=True,
                         check=True).stdout.splitlines()
    plan = [int(t) for t in out[0].split()[1:]]
    got = {k: np.full(lens[k], np.nan) for k in names}
    count = {k: np.zeros(lens[k], dtype=int) for k in names}
    for line in out[1:]:
        _, seq, idx, val = line.split()
        k = names[int(seq)]
        assert 0 <= int(idx) < lens[k], (k, idx)
        got[k][int(idx)] = float(val)
        count[k][int(idx)] += 1
    split = lambda M: (M[:, :nz], M[:, nz:nz + nl], M[:, nz + nl:])
    return plan, got, count, split(X), split(P)


def _check_plan_line(plan, batch):
    tiles, chunk, slot, chunks, scratch = plan
    # include/fbstab_hip.h: tiles x ceil(batch / 128) x 272 doubles
    assert (chunk, slot) == (128, 272) == (R.chunk(), R.plan_constant("kGradReduceSlot"))
    assert chunks == -(-batch // chunk) and scratch == tiles * chunks * slot
    return tiles


@pytest.mark.parametrize("shape", R.DENSE_SHAPES)
def test_dense_table_walk_matches_the_numpy_table_and_covers_every_entry_once(driver, shape):
    nz, nl, nv = shape
    lens = R.dense_lens(*shape)
    plan, got, count, x, step = _walk(driver, "dense", shape, lens, DENSE_ARR)
    tiles = _check_plan_line(plan, BATCH)
    assert tiles == -(-(nz + nl + nv) // 16) * -(-nz // 16)
    ref = {k: np.zeros(lens[k]) for k in DENSE_ARR}
    for b in range(BATCH):
        tab = LR.dense_gradient_table(nz, nl, nv, [t[b] for t in x], [t[b] for t in step])
        for k in DENSE_ARR:
            ref[k] += tab[k]
    for k in DENSE_ARR:
        assert (count[k] == 1).all(), (k, count[k].min(), count[k].max())
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-13, err_msg=k)
        # ... and the extended-precision table of the GPU tests says the same, within their bound
        R.check_sum(k, got[k], R.dense_sum_table(nz, nl, nv, x, step)[k], BATCH)


def _mpc_table_one_qp(N, nx, nu, nc, x, step):
    """fb_adjoint.h's table for ONE QP, entry by entry as mpc_adjoint_contract indexes it."""
    z, l, v = x
    dz, dl, dv = step
    ns = nx + nu
    lens = R.mpc_lens(N, nx, nu, nc)
    G = {k: np.zeros(lens[k]) for k in MPC_SEQ}
    for i in range(N + 1):
        xs, dxs, us, dus = z[i * ns:i * ns + nx], dz[i * ns:i * ns + nx], z[i * ns + nx:(i + 1) * ns], dz[i * ns + nx:(i + 1) * ns]
        vi, dvi = v[i * nc:(i + 1) * nc], dv[i * nc:(i + 1) * nc]
        for k in range(nx):
            for r in range(nx):
                G["Q"][i * nx * nx + r + k * nx] = -0.5 * (dxs[r] * xs[k] + xs[r] * dxs[k])
            for r in range(nu):
                G["S"][i * nu * nx + r + k * nu] = -(dus[r] * xs[k] + us[r] * dxs[k])
            for r in range(nc):
                G["E"][i * nc * nx + r + k * nc] = -(dvi[r] * xs[k] + vi[r] * dxs[k])
        for k in range(nu):
            for r in range(nu):
                G["R"][i * nu * nu + r + k * nu] = -0.5 * (dus[r] * us[k] + us[r] * dus[k])
            for r in range(nc):
                G["L"][i * nc * nu + r + k * nc] = -(dvi[r] * us[k] + vi[r] * dus[k])
        G["q"][i * nx:(i + 1) * nx] = -dxs
        G["r"][i * nu:(i + 1) * nu] = -dus
        G["d"][i * nc:(i + 1) * nc] = -dvi
        if i < N:
            lp, dlp = l[(i + 1) * nx:(i + 2) * nx], dl[(i + 1) * nx:(i + 2) * nx]
            for r in range(nx):
                for k in range(nx):
                    G["A"][i * nx * nx + r + k * nx] = -(dlp[r] * xs[k] + lp[r] * dxs[k])
                for k in range(nu):
                    G["B"][i * nx * nu + r + k * nx] = -(dlp[r] * us[k] + lp[r] * dus[k])
            G["c"][i * nx:(i + 1) * nx] = -dlp
    G["x0"][:] = -dl[:nx]
    return G


@pytest.mark.parametrize("shape", R.MPC_SHAPES)
def test_mpc_table_walk_matches_the_numpy_table_and_covers_every_entry_once(driver, shape):
    N, nx, nu, nc = shape
    lens = R.mpc_lens(*shape)
    plan, got, count, x, step = _walk(driver, "mpc", shape, lens, MPC_SEQ)
    tiles = _check_plan_line(plan, BATCH)
    ns, up = nx + nu, lambda a: -(-a // 16)
    assert tiles == N * up(ns + nx + nc) * up(ns) + up(ns + nc) * up(ns) + up(nx)
    ref = {k: np.zeros(lens[k]) for k in MPC_SEQ}
    for b in range(BATCH):
        tab = _mpc_table_one_qp(N, nx, nu, nc, [t[b] for t in x], [t[b] for t in step])
        for k in MPC_SEQ:
            ref[k] += tab[k]
    summed = R.mpc_sum_table(N, nx, nu, nc, x, step)
    for k in MPC_SEQ:
        assert (count[k] == 1).all(), (k, count[k].min(), count[k].max())
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-13, err_msg=k)
        R.check_sum(k, got[k], summed[k], BATCH)


def test_scratch_sizes_are_the_documented_ones(driver):
    """include/fbstab_hip.h: 94 tiles and 13.1 MB of partial sums at the headline shape and max_batch 8192, 40
    tiles and 2.8 MB at (50, 10, 100) and 4096 (and 97.5 MB / 5.2 MB of adjoint steps, max_batch x (nz + nl + nv))."""
    plan, *_ = _walk(driver, "mpc", (30, 12, 4, 20), R.mpc_lens(30, 12, 4, 20), MPC_SEQ, batch=1)
    assert plan[0] == 94 and round(94 * (8192 // 128) * 272 * 8 / 1e6, 1) == 13.1
    assert round(8192 * 31 * (16 + 12 + 20) * 8 / 1e6, 1) == 97.5
    plan, *_ = _walk(driver, "dense", (50, 10, 100), R.dense_lens(50, 10, 100), DENSE_ARR, batch=1)
    assert plan[0] == 40 and round(40 * (4096 // 128) * 272 * 8 / 1e6, 1) == 2.8
    # a batch that is no multiple of the chunk: the last chunk is short, not dropped
    plan, *_ = _walk(driver, "dense", (5, 2, 9), R.dense_lens(5, 2, 9), DENSE_ARR, batch=129)
    assert plan[3] == 2 and plan[4] == plan[0] * 2 * 272


def test_reduced_entry_points_validate_without_a_device():
    """In the order of test_argument_validation_without_gpu: NULL argument blocks, a NULL z seed, a gradient stride
    strictly between 0 and the length with batch > 1 - each FBSTAB_HIP_ERR_ARGUMENT before any device call (there
    is no handle: nothing can have been created without a device either)."""
    from fbstab_amd import hip_api
    lib = hip_api.load_library()
    buf = np.zeros(64)
    st = np.zeros(4, dtype=np.int32)

    def call(kind, batch, blocks=True, seed_z=True, grad_stride=8):
        b = hip_api._MpcBatch() if kind == "mpc" else hip_api._DenseBatch()
        g = hip_api._MpcGradBatch() if kind == "mpc" else hip_api._DenseGradBatch()
        x, s = hip_api._VarBatch(), hip_api._VarBatch()
        for i in range(len(b.base)):
            b.base[i], b.stride[i] = buf.ctypes.data, 8
        for i in range(3):
            x.base[i], x.stride[i] = buf.ctypes.data, 8
        if seed_z:
            s.base[0], s.stride[0] = buf.ctypes.data, 8
        g.base[1], g.stride[1] = buf.ctypes.data, grad_stride
        fn = getattr(lib, "fbstab_hip_%s_adjoint_batch_reduced" % kind)
        if not blocks:
            return fn(None, batch, None, None, None, 0.0, None, None, None, None, 0, None), lib.fbstab_hip_last_error()
        rc = fn(None, batch, C.byref(b), C.byref(x), C.byref(s), 0.0, C.byref(g), None, st.ctypes.data, None, 0, None)
        return rc, lib.fbstab_hip_last_error()

    for kind in ("mpc", "dense"):
        assert call(kind, 1, blocks=False)[0] == 1
        assert call(kind, 1, seed_z=False)[0] == 1
        assert call(kind, 2, grad_stride=-1)[0] == 1
        assert call(kind, 2, grad_stride=1)[0] == 1   # 0 < stride < length for every shape but length 1
        assert call(kind, 2, grad_stride=0)[0] == 1   # (a reduced slot: accepted; what stops the call is the handle)
    # the dense entry point knows these before it looks at the handle
    rc, msg = call("dense", 1, blocks=False)
    assert rc == 1 and b"null argument" in msg
    rc, msg = call("dense", 1, seed_z=False)
    assert rc == 1 and b"null seed pointer (z)" in msg
    rc, msg = call("dense", 2, grad_stride=-1)
    assert rc == 1 and b"gradient stride smaller than the array length" in msg
    rc, msg = call("dense", 2, grad_stride=0)
    assert rc == 1 and b"null solver handle" in msg
    # ... and fbstab_hip_dense_adjoint_batch still refuses the stride 0 that the reduced call accepts
    b, g, x, s = hip_api._DenseBatch(), hip_api._DenseGradBatch(), hip_api._VarBatch(), hip_api._VarBatch()
    for i in range(6):
        b.base[i], b.stride[i] = buf.ctypes.data, 8
    for i in range(3):
        x.base[i], x.stride[i] = buf.ctypes.data, 8
    s.base[0], s.stride[0] = buf.ctypes.data, 8
    g.base[1], g.stride[1] = buf.ctypes.data, 0
    rc = lib.fbstab_hip_dense_adjoint_batch(None, 2, C.byref(b), C.byref(x), C.byref(s), 0.0, C.byref(g), None,
                                            st.ctypes.data, 0, None)
    assert rc == 1 and b"gradient stride smaller than the array length" in lib.fbstab_hip_last_error()
