// Dynamic-LDS layouts of the EKF kernels, written once: the launcher takes the byte count of a launch and the kernel carves its pointers
// from the same description (offsets in doubles from the base of the dynamic region). Plain C++: no HIP header, so a host compiler
// alone can build it (tests/cpp/test_lds_layout.cpp).
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define HV_HD __host__ __device__ __attribute__((always_inline))
#else
#define HV_HD
#endif

namespace hv {

// ---- the CU's LDS and the kernels' dynamic-LDS limits (set once per context: ekf_kernels_init) ----
constexpr size_t LDS_CU_BYTES = 160 * 1024;
constexpr size_t LDS_DEFAULT_LIMIT = 64 * 1024;            // what a kernel gets without a raised limit (ekf_augment_kernel<true> stays there)
constexpr size_t LDS_UPDATE_LIMIT = LDS_CU_BYTES;          // update kernels, one workgroup per CU: T alone reaches 154 KB at 80 rows (20 stereo poses)
constexpr size_t LDS_GATE_LIMIT = 96 * 1024;               // streaming gate and small sparse gate: up to three workgroups per CU
constexpr size_t LDS_SGATE_BIG_LIMIT = LDS_CU_BYTES - 64;  // big sparse gate: its turn counters are 32 bytes of STATIC LDS beside the dynamic part
constexpr size_t LDS_AUGMENT_LIMIT = 158 * 1024;           // augmentation of states with map points (n > ~190)

// Column stride of a column-major LDS matrix of `rows` rows: the next count that is 15 or 17 mod 32 doubles. Odd keeps the 16 lanes of
// a row-strided operand read (S = HP H') in distinct banks; 2 Rs = 30 or 34 mod 64 dwords puts the k-groups of a column-strided read
// (the Cholesky panels, Y'Y) half a bank array apart.
HV_HD constexpr int lds_stride(int rows)
{
    while ((rows & 31) != 15 && (rows & 31) != 17) rows++;
    return rows;
}
HV_HD constexpr int lds_stride_tight(int rows) { return rows + ((rows & 1) ? 0 : 1); }    // where LDS does not allow that (84-row tracks): the next odd count
HV_HD constexpr int tiles16(int x) { return (x + 15) >> 4; }
template <class L> HV_HD constexpr size_t lds_bytes(const L &l) { return sizeof(double) * (size_t)l.end; }

// ---- scratch of the blocked Cholesky (factor_diag_block, gate_factor_chi2): W[256] | col[544] | red[waves] ----
// W: inverse of the current 16 x 16 diagonal block; col: column broadcast buffer of the diagonal factor, col[256 .. 527] the dump area of
// its branch-free stores; red: one partial sum per wavefront
constexpr int CHOL_W = 0, CHOL_COL = CHOL_W + 256, CHOL_RED = CHOL_COL + 544;
HV_HD constexpr int chol_scratch_doubles(int nwaves) { return CHOL_RED + nwaves; }
constexpr int CHOL_SCRATCH_FLOOR = 824;    // least size of a region that the scratch borrows later (the widest workgroup has 16 wavefronts)
static_assert(CHOL_SCRATCH_FLOOR >= chol_scratch_doubles(16) && CHOL_SCRATCH_FLOOR % 2 == 0, "the floor must hold the scratch of every kernel");

// ---- update (ekf_update_kernel and its dual / spec-long forms): T | W col red | flag[2] | Hs ----
// T: the tall matrix, Rs x nr (rounded to an even count: what follows stays 16-byte aligned); in kernel mode 0 it lives in a global
// workspace and the carve starts at the scratch. Hs (mode 2 only): H zero-padded to (16 ti) x (16 lbk).
struct UpdateLds { size_t T, chol, red, flag, Hs, end; };
HV_HD constexpr UpdateLds update_lds(int Rs, int nr, int nwaves, bool t_in_lds, size_t hs_doubles)
{
    const size_t chol = t_in_lds ? (((size_t)Rs * nr + 1) & ~(size_t)1) : 0, red = chol + CHOL_RED, flag = red + nwaves, Hs = flag + 2;
    return UpdateLds{0, chol, red, flag, Hs, Hs + hs_doubles};
}
// The launch's shape: kernel mode 0 = T in a global workspace (no padding), 1 = T in LDS and H streamed from L2, 2 = H staged in LDS as
// well (n <= 160, at most 48 rows; hs: its doubles). two_r: a mode-2 launch can park S and v in the H area (UpdateRequest::mode 3).
struct UpdateShape { int Rs, kmode, ti, lbk; size_t hs; bool two_r; };
HV_HD constexpr UpdateShape update_shape(int n, int nr, int l, int nwaves)
{
    UpdateShape s{lds_stride(nr + n + 1), 0, tiles16(nr), tiles16(l), 0, false};
    s.hs = (size_t)(16 * s.ti) * (16 * s.lbk);
    if (lds_bytes(update_lds(s.Rs, nr, nwaves, true, 0)) > LDS_UPDATE_LIMIT) { s.Rs = nr + n + 1; return s; }
    s.kmode = (n <= 160 && nr <= 48 && lds_bytes(update_lds(s.Rs, nr, nwaves, true, s.hs)) <= LDS_UPDATE_LIMIT) ? 2 : 1;
    s.two_r = s.kmode == 2 && (size_t)(nr + 1) * nr + 256 <= s.hs;
    return s;
}

// ---- streaming gate (ekf_gate_stream_kernel): Hs | T (+ 2 spare); the Cholesky scratch borrows Hs once the products are done ----
// Hs: H zero-padded, (16 ti) x (16 lbk), k-major; T: [S; v'], (nr + 1) x nr at stride Rs
struct GateStreamLds { size_t Hs, T, end; };
HV_HD constexpr GateStreamLds gate_stream_lds(int ti, int lbk, int Rs, int nr)
{
    const size_t T = (size_t)(16 * ti) * 16 * lbk;
    return GateStreamLds{0, T, T + (size_t)Rs * nr + 2};
}
// (Hs is a multiple of 256 doubles: the floor declines exactly the shapes with ti * lbk <= 3)
HV_HD constexpr bool gate_stream_admitted(const GateStreamLds &L) { return L.T - L.Hs >= (size_t)CHOL_SCRATCH_FLOOR && lds_bytes(L) <= LDS_GATE_LIMIT; }

// ---- sparse gate (ekf_sparse_gate_kernel: <= 48 rows, ekf_sparse_gate_big_kernel: 49 .. 96): Hs | T | acol (ints) ----
// Hs: the compact Jacobian staged k-major, na4 columns of nrp rows (>= CHOL_SCRATCH_FLOOR: the scratch borrows it); T: [S; v'].
// A launch is sized for its longest record. In the big build a record whose padded layout (nrp = 16 ti, stride lds_stride) does not fit
// uses the tight one (nrp = 84, odd stride) inside the same carve.
constexpr int HV_GATE_TIGHT_ROWS = 84;     // rows per staged column of the tight layout: 21 stereo poses, the longest track there is
struct SparseGateShape { int Rs, nrp; bool tight; };
HV_HD constexpr SparseGateShape sparse_gate_shape(bool big, int nr, int na4, size_t budget_doubles)       // one record's, within Hs + T doubles
{
    const int t = tiles16(nr), ti = big ? (t > 4 ? t : 4) : t;     // (the big build starts at the 4-tile instantiation)
    int Rs = lds_stride(nr + 1);
    const bool tight = big && (size_t)na4 * 16 * ti + (size_t)Rs * nr > budget_doubles;
    if (tight) Rs = lds_stride_tight(nr + 1);
    return SparseGateShape{Rs, tight ? HV_GATE_TIGHT_ROWS : 16 * ti, tight};
}
struct SparseGateLds { SparseGateShape shape; bool big, supported; size_t Hs, T, acol, bytes; };    // acol: doubles in front of the int list [na_max + 2]
HV_HD constexpr SparseGateLds sparse_gate_lds(int np, int ncam)         // the launch's, for records of up to np poses on ncam cameras
{
    const int nr = 2 * np * ncam, na_max = 7 * np + 1, na4 = (na_max + 3) & ~3;
    const bool big = nr > 48;
    const size_t limit = big ? LDS_SGATE_BIG_LIMIT : LDS_GATE_LIMIT, ints = sizeof(int) * (size_t)(na_max + 2);
    const SparseGateShape s = sparse_gate_shape(big, nr, na4, (limit - ints) / sizeof(double));
    const size_t hc = (size_t)na4 * s.nrp, hs = hc < (size_t)CHOL_SCRATCH_FLOOR ? CHOL_SCRATCH_FLOOR : hc;
    // (the tight T is reserved at the even stride nr + 2, the (84 + 2) x 84 of VuLds::LONG_T; the kernel's odd stride leaves its tail unused)
    const size_t acol = hs + (s.tight ? (size_t)(nr + 2) * nr : (size_t)s.Rs * nr), bytes = sizeof(double) * acol + ints;
    return SparseGateLds{s, big, !(s.tight && nr > HV_GATE_TIGHT_ROWS) && bytes <= limit, 0, hs, acol, bytes};
}

// ---- augmentation (ekf_augment_kernel): HP | K | G | S0 | Lc | vres | scratch ----
// [HP | K | G]: 7 x n each, row-major and contiguous (rows 0..13 are the MFMA A operand, rows 7..20 the B operand of step 4); S0, Lc: 7 x 7;
// vres: 7 (+ 1); scratch: one 16 x 17 transpose tile per wavefront, then Wc (n x 14, at `scratch`) | T14 (14 x 14)
constexpr int AUG_POSE = 7, AUG_J = 2 * AUG_POSE;
struct AugmentLds { int HP, K, G, S0, Lc, vres, scratch, T14, end; };
HV_HD constexpr AugmentLds augment_lds(int n, int nwaves)
{
    const int row = AUG_POSE * n, sq = AUG_POSE * AUG_POSE, scratch = 3 * row + 2 * sq + AUG_POSE + 1;
    const int transposes = nwaves * 16 * 17, wc_t14 = AUG_J * n + AUG_J * AUG_J;
    return AugmentLds{0, row, 2 * row, 3 * row, 3 * row + sq, 3 * row + 2 * sq, scratch, scratch + AUG_J * n, scratch + (transposes > wc_t14 ? transposes : wc_t14)};
}

}  // namespace hv
