// One QP's share of a batch block.  The kernels take the blocks of include/fbstab_hip.h as they are - one base
// pointer and one stride (in doubles) per array, QP q at base + q * stride - and these helpers are the one place
// where a block and a QP index become pointers: a single slot, the z / l / v / y slots of a variable block, or the
// named-pointer structs the numerics work on.  Two forms of each:
//   *_at        plain base + q * stride: the slot is there (problem data and iterates of a solve)
//   *_or_null   a null base stays null: the slot is optional (gradients, perturbations, seeds, adjoints)
// Well-formed on the host too (tests/hostsim).
#pragma once

#include "../../include/fbstab_hip.h"
#include "fb_common.h"

namespace fbk {

// Pointers to one QP's problem data (already offset to that QP) ...
struct MpcData {
  const double *Q, *R, *S, *q, *r, *A, *B, *c, *E, *L, *d, *x0;
};
struct DenseData {
  const double *H, *f, *G, *h, *A, *b;
};
// ... to its perturbations (fb_tangent.h; nullptr: zero) ...
typedef MpcData MpcDir;
typedef DenseData DenseDir;
// ... and to its gradients (fb_adjoint.h; nullptr: not wanted), in the order of fbstab_mpc_batch_t and
// fbstab_dense_batch_t.
struct MpcGrad {
  double *Q, *R, *S, *q, *r, *A, *B, *c, *E, *L, *d, *x0;
};
struct DenseGrad {
  double *H, *f, *G, *h, *A, *b;
};

template <class T>
FB_DEV T* slot_at(T* base, long long stride, long q) { return base + q * stride; }
template <class T>
FB_DEV T* slot_or_null(T* base, long long stride, long q) { return base ? base + q * stride : nullptr; }

// Slot i (0 .. 3: z, l, v, y) of a variable block.
FB_DEV double* var_at(const fbstab_var_batch_t& x, int i, long q) { return slot_at(x.base[i], x.stride[i], q); }
FB_DEV double* var_or_null(const fbstab_var_batch_t& x, int i, long q) {
  return slot_or_null(x.base[i], x.stride[i], q);
}

// Out: MpcData or MpcGrad from fbstab_mpc_batch_t or fbstab_mpc_grad_batch_t; NULLS: the null-tolerant form.
template <class Out, bool NULLS, class Block>
FB_DEV Out mpc_slots(const Block& b, long q) {
#define FB_SLOT(name) \
  o.name = NULLS ? slot_or_null(b.base[FBSTAB_MPC_##name], b.stride[FBSTAB_MPC_##name], q) \
                 : slot_at(b.base[FBSTAB_MPC_##name], b.stride[FBSTAB_MPC_##name], q)
  Out o;
  FB_SLOT(Q); FB_SLOT(R); FB_SLOT(S); FB_SLOT(q); FB_SLOT(r); FB_SLOT(A);
  FB_SLOT(B); FB_SLOT(c); FB_SLOT(E); FB_SLOT(L); FB_SLOT(d); FB_SLOT(x0);
#undef FB_SLOT
  return o;
}
template <class Out, bool NULLS, class Block>
FB_DEV Out dense_slots(const Block& b, long q) {
#define FB_SLOT(name) \
  o.name = NULLS ? slot_or_null(b.base[FBSTAB_DENSE_##name], b.stride[FBSTAB_DENSE_##name], q) \
                 : slot_at(b.base[FBSTAB_DENSE_##name], b.stride[FBSTAB_DENSE_##name], q)
  Out o;
  FB_SLOT(H); FB_SLOT(f); FB_SLOT(G); FB_SLOT(h); FB_SLOT(A); FB_SLOT(b);
#undef FB_SLOT
  return o;
}

FB_DEV MpcData mpc_data_at(const fbstab_mpc_batch_t& d, long q) { return mpc_slots<MpcData, false>(d, q); }
FB_DEV MpcData mpc_data_or_null(const fbstab_mpc_batch_t& d, long q) { return mpc_slots<MpcData, true>(d, q); }
FB_DEV MpcGrad mpc_grad_or_null(const fbstab_mpc_grad_batch_t& g, long q) { return mpc_slots<MpcGrad, true>(g, q); }
FB_DEV DenseData dense_data_at(const fbstab_dense_batch_t& d, long q) { return dense_slots<DenseData, false>(d, q); }
FB_DEV DenseData dense_data_or_null(const fbstab_dense_batch_t& d, long q) {
  return dense_slots<DenseData, true>(d, q);
}
FB_DEV DenseGrad dense_grad_or_null(const fbstab_dense_grad_batch_t& g, long q) {
  return dense_slots<DenseGrad, true>(g, q);
}

}  // namespace fbk
