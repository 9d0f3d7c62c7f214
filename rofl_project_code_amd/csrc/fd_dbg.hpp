// One op table over the register-radix arithmetic of fe26.hpp and the scalar field of fe32.hpp, compiled for the device (k_dbg_fd /
// k_dbg_sc in kernels.hpp) and for the host (rofl_dbg_host_fd_ops_raw / rofl_dbg_host_sc_ops, with the bound assertions of
// ROFL_FD_CHECK on).  Operands and results are RAW limb arrays: the caller chooses the representation of a value, not only the value,
// and sees the tightness of every result.  tests/fd_model.py holds the exact model and the corpus; include/rofl_zk_debug.h documents
// the layout.  Nothing in production includes a function of this file.
#pragma once
#include "fe26.hpp"

namespace rofl {

#define FD_DBG_IN 80       // u32 per case, operands: up to 8 field elements of 10 limbs
#define FD_DBG_OUT 80      // u32 per case, results
enum { FD_DBG_UNPACK = 0, FD_DBG_CARRY = 1, FD_DBG_PACK = 2, FD_DBG_ADD = 3, FD_DBG_SUB = 4, FD_DBG_NEG = 5, FD_DBG_MUL = 6, FD_DBG_SQ = 7,
       FD_DBG_MUL_LOOSE = 8, FD_DBG_SQ_LOOSE = 9, FD_DBG_INVERT = 10, FD_DBG_POW22523 = 11, FD_DBG_SQRT_RATIO = 12, FD_DBG_ABS = 13,
       FD_DBG_PRED = 14, FD_DBG_MADD = 15, FD_DBG_MSUB = 16, FD_DBG_GD_ADD = 17, FD_DBG_GD_DOUBLE = 18, FD_DBG_GD_DOUBLE_NOT = 19,
       FD_DBG_TO_NIELS = 20, FD_DBG_TO_NIELS_ZINV = 21, FD_DBG_THREAD_OPS = 22,
       FD_DBG_GQ_DOUBLE = 22, FD_DBG_GQ_ADD = 23, FD_DBG_OPS = 24 };       // 22, 23: one quad of lanes per case, device only

HD fd fd_dbg_load(const u32 *in, int k) {
    fd r;
#pragma unroll
    for (int i = 0; i < 10; i++) r.v[i] = in[10 * k + i];
    return r;
}
HD void fd_dbg_store(u32 *out, int k, const fd &a) {
#pragma unroll
    for (int i = 0; i < 10; i++) out[10 * k + i] = a.v[i];
}
HD gd gd_dbg_load(const u32 *in, int k) { gd r; r.X = fd_dbg_load(in, k); r.Y = fd_dbg_load(in, k + 1); r.Z = fd_dbg_load(in, k + 2); r.T = fd_dbg_load(in, k + 3); return r; }
HD void gd_dbg_store(u32 *out, int k, const gd &p) { fd_dbg_store(out, k, p.X); fd_dbg_store(out, k + 1, p.Y); fd_dbg_store(out, k + 2, p.Z); fd_dbg_store(out, k + 3, p.T); }
HD void fe_dbg_store(u32 *out, int w, const fe &a) {
#pragma unroll
    for (int i = 0; i < 8; i++) out[w + i] = a.v[i];
}
HD void niels_dbg_store(u32 *out, const niels &q) { fe_dbg_store(out, 0, q.ypx); fe_dbg_store(out, 8, q.ymx); fe_dbg_store(out, 16, q.t2d); }

// `in`: FD_DBG_IN words, `out`: FD_DBG_OUT words (words an op does not write keep what the caller put there)
HDN inline void fd_dbg_apply(u32 op, const u32 *in, u32 *out) {
    switch (op) {
    case FD_DBG_UNPACK: { fe w; for (int i = 0; i < 8; i++) w.v[i] = in[i]; fd_dbg_store(out, 0, fd_unpack(w)); break; }
    case FD_DBG_CARRY: fd_dbg_store(out, 0, fd_carry(fd_dbg_load(in, 0))); break;
    case FD_DBG_PACK: {
        fe w = fd_pack(fd_dbg_load(in, 0));
        uint8_t b[32]; fe_tobytes(b, w);
        fe_dbg_store(out, 0, w);
        for (int i = 0; i < 8; i++) out[8 + i] = (u32)b[4 * i] | ((u32)b[4 * i + 1] << 8) | ((u32)b[4 * i + 2] << 16) | ((u32)b[4 * i + 3] << 24);
        break;
    }
    case FD_DBG_ADD: fd_dbg_store(out, 0, fd_add(fd_dbg_load(in, 0), fd_dbg_load(in, 1))); break;
    case FD_DBG_SUB: fd_dbg_store(out, 0, fd_sub(fd_dbg_load(in, 0), fd_dbg_load(in, 1))); break;
    case FD_DBG_NEG: fd_dbg_store(out, 0, fd_neg(fd_dbg_load(in, 0))); break;
    case FD_DBG_MUL: fd_dbg_store(out, 0, fd_mul(fd_dbg_load(in, 0), fd_dbg_load(in, 1))); break;
    case FD_DBG_SQ: fd_dbg_store(out, 0, fd_sq(fd_dbg_load(in, 0))); break;
    case FD_DBG_MUL_LOOSE: fd_dbg_store(out, 0, fd_mul(fd_sub(fd_dbg_load(in, 0), fd_dbg_load(in, 1)), fd_add(fd_dbg_load(in, 2), fd_dbg_load(in, 3)))); break;
    case FD_DBG_SQ_LOOSE: fd_dbg_store(out, 0, fd_sq(fd_add(fd_dbg_load(in, 0), fd_dbg_load(in, 1)))); break;
    case FD_DBG_INVERT: fd_dbg_store(out, 0, fd_invert(fd_dbg_load(in, 0))); break;
    case FD_DBG_POW22523: fd_dbg_store(out, 0, fd_pow22523(fd_dbg_load(in, 0))); break;
    case FD_DBG_SQRT_RATIO: { fd r; bool sq = fd_sqrt_ratio_i(r, fd_dbg_load(in, 0), fd_dbg_load(in, 1)); fd_dbg_store(out, 0, r); out[10] = sq ? 1u : 0u; break; }
    case FD_DBG_ABS: fd_dbg_store(out, 0, fd_abs(fd_dbg_load(in, 0))); break;
    case FD_DBG_PRED: {
        fd a = fd_dbg_load(in, 0), b = fd_dbg_load(in, 1);
        out[0] = fd_isneg(a) ? 1u : 0u; out[1] = fd_iszero(a) ? 1u : 0u; out[2] = fd_eq(a, b) ? 1u : 0u;
        break;
    }
    case FD_DBG_MADD: case FD_DBG_MSUB: {
        nd q; q.ypx = fd_dbg_load(in, 4); q.ymx = fd_dbg_load(in, 5); q.t2d = fd_dbg_load(in, 6);
        gd_dbg_store(out, 0, gd_madd(gd_dbg_load(in, 0), q, op == FD_DBG_MSUB));
        break;
    }
    case FD_DBG_GD_ADD: gd_dbg_store(out, 0, gd_add(gd_dbg_load(in, 0), gd_dbg_load(in, 4))); break;
    case FD_DBG_GD_DOUBLE: gd_dbg_store(out, 0, gd_double(gd_dbg_load(in, 0))); break;
    case FD_DBG_GD_DOUBLE_NOT: gd_dbg_store(out, 0, gd_double_not(gd_dbg_load(in, 0))); break;
    case FD_DBG_TO_NIELS: niels_dbg_store(out, gd_to_niels(gd_dbg_load(in, 0))); break;
    case FD_DBG_TO_NIELS_ZINV: niels_dbg_store(out, gd_to_niels_zinv(gd_dbg_load(in, 0), fd_dbg_load(in, 4))); break;
    default: break;
    }
}

// ---------------------------------------------------------------- scalar field
#define SC_DBG_IN 264      // u32 per case: 32 scalars of 8 words, then the product count of SC_DBG_MAC in word 256 (16-byte aligned stride)
#define SC_DBG_OUT 8
enum { SC_DBG_MONTMUL = 0, SC_DBG_TO_MONT = 1, SC_DBG_FROM_MONT = 2, SC_DBG_MUL_PLAIN = 3, SC_DBG_ADD = 4, SC_DBG_NEG = 5, SC_DBG_SUB = 6,
       SC_DBG_LOAD_REDUCED = 7,      // kernels.hpp's load_sc_reduced on the device; the host twin spells out the same two steps
       SC_DBG_FROM_WIDE = 8, SC_DBG_FROM_WIDE_MONT = 9, SC_DBG_MAC = 10, SC_DBG_INVERT_MONT = 11, SC_DBG_OPS = 12 };

HD sc sc_dbg_load(const u32 *in, int k) {
    sc r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = in[8 * k + i];
    return r;
}
HDN inline sc sc_dbg_apply(u32 op, const u32 *in) {
    const sc a = sc_dbg_load(in, 0), b = sc_dbg_load(in, 1);
    switch (op) {
    case SC_DBG_MONTMUL: return sc_montmul(a, b);
    case SC_DBG_TO_MONT: return sc_to_mont(a);
    case SC_DBG_FROM_MONT: return sc_from_mont(a);
    case SC_DBG_MUL_PLAIN: return sc_mul_plain(a, b);
    case SC_DBG_ADD: return sc_add(a, b);
    case SC_DBG_NEG: return sc_neg(a);
    case SC_DBG_SUB: return sc_sub(a, b);
    case SC_DBG_LOAD_REDUCED: return sc_geq_l(a.v) ? sc_from_mont(sc_to_mont(a)) : a;
    case SC_DBG_FROM_WIDE: return sc_from_wide(a, b);
    case SC_DBG_FROM_WIDE_MONT: return sc_from_wide_mont(a, b);
    case SC_DBG_MAC: {
        u32 acc[17]; for (int i = 0; i < 17; i++) acc[i] = 0;
        u32 count = in[256] > 16 ? 16 : in[256];
        for (u32 k = 0; k < count; k++) sc_mac_wide(acc, sc_dbg_load(in, 2 * (int)k), sc_dbg_load(in, 2 * (int)k + 1));
        return sc_redc_wide(acc);
    }
    case SC_DBG_INVERT_MONT: return sc_invert_mont(a);
    default: return sc_zero();
    }
}

}  // namespace rofl
