// Host orchestration of one STARK proof: the GPU counterpart of the reference's
//   starks::common::prover::prove                 src/starks/common/prover.rs:18-72
// followed by starky's prove_with_commitment, as called from G1StarkProofGenerator::run_once
// (src/generators/g1/stark_proof.rs:151-163).  All polynomial data stays in HBM; the host only runs the
// Fiat-Shamir transcript on caps / openings (a few KB per round trip) and assembles the proof words.
//
// In this file, in the order a proof meets them:
//   stark_kind()         what differs between the three STARKs, one table (prover.h);
//   proof_plan()         everything decided before memory is touched, the workspace layout above all (proof_plan.h / .hip);
//   Workspace            the named buffers of the slot, acquired from the plan (workspace_acquire);
//   Transforms           iNTT / LDE dispatch by trace height and workspace (transforms.h);
//   stage_* / commit()   the stages, one function each; the pieces that are host arithmetic alone (opening recombination,
//                        alpha powers, final polynomial, assembly of the words) are free functions without a HIP call;
//   prove_on_slot()      the list of stages with the transcript between them;
//   the C ABI            batches on the worker pool, the out-of-memory retry, accessors.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>
#include "ctx.h"
#include "trace.h"
#include "aux.h"
#include "merkle.h"
#include "quotient.h"
#include "fri.h"
#include "transcript.h"
#include "prover.h"
#include "proof_plan.h"
#include "transforms.h"

// ---- the three kinds -------------------------------------------------------------------------------------------
// Stark::lookups (range-checked columns), the two looked CTL tables and the constraint counts of the three AIRs:
// G1 scalar_mul_{view,stark,ctl}.rs, G2 twins, fields/exp_{view,stark,ctl}.rs.
template <class L>
static StarkShape make_shape(bool input_has_a, int n_constraints) {
  StarkShape s;
  s.W = L::W;
  s.rc_begin = L::RC_BEGIN;
  s.rc_end = L::RC_END;
  s.table_col = L::RANGE;
  s.freq_col = L::FREQ;
  s.n_ctl = 2;
  s.n_constraints = n_constraints;
  memset(&s.ctl, 0, sizeof(s.ctl));
  int m = 0;
  for (int i = 0; i < L::PL; i++, m++) { s.ctl.col_start[0][m] = L::B + i; s.ctl.col_bits[0][m] = 1; }
  if (input_has_a)
    for (int i = 0; i < L::PL; i++, m++) { s.ctl.col_start[0][m] = L::A + i; s.ctl.col_bits[0][m] = 1; }
  for (int k = 0; k < 16; k++, m++) { s.ctl.col_start[0][m] = L::BITS + 16 * k; s.ctl.col_bits[0][m] = 16; }
  s.ctl.col_start[0][m] = L::TIMESTAMP; s.ctl.col_bits[0][m] = 1; m++;
  s.ctl.ncols[0] = m;
  s.ctl.filter_col[0] = L::FLAGS + 0;
  m = 0;
  for (int i = 0; i < L::PL; i++, m++) { s.ctl.col_start[1][m] = L::SUM + i; s.ctl.col_bits[1][m] = 1; }
  s.ctl.col_start[1][m] = L::TIMESTAMP; s.ctl.col_bits[1][m] = 1; m++;
  s.ctl.ncols[1] = m;
  s.ctl.filter_col[1] = L::FLAGS + 1;
  return s;
}
static int fq_generate_trace_no_offset(const u64* d_scalars, const u64* d_x, const u64*, size_t n, u64* d_trace, size_t N,
                                       u64* d_scratch, u64* d_outputs, int* d_err, hipStream_t st, bool with_range) {
  return fq_generate_trace_device(d_scalars, d_x, n, d_trace, N, d_scratch, d_outputs, d_err, st, with_range);
}
const StarkKind& stark_kind(int kind) {
  static const StarkKind kinds[3] = {
      {make_shape<G1L>(true, 1111), 8, true, g1_trace_scratch_words, g1_generate_trace_device, g1_quotient_mz_blocks, g1_quotient_launch},
      {make_shape<G2L>(true, 1693), 16, true, g2_trace_scratch_words, g2_generate_trace_device, g2_quotient_mz_blocks, g2_quotient_launch},
      {make_shape<FQL>(false, 770), 4, false, fq_trace_scratch_words, fq_generate_trace_no_offset, fq_quotient_mz_blocks, fq_quotient_launch}};
  return kinds[kind];
}

// ---- proof object ---------------------------------------------------------------------------------------------
enum { ST_TRACE = 0, ST_TRACE_NTT, ST_TRACE_MERKLE, ST_AUX, ST_AUX_NTT, ST_AUX_MERKLE, ST_QUOTIENT, ST_QUOTIENT_COMMIT,
       ST_OPENINGS, ST_FRI, ST_TOTAL, ST_COUNT };
static const char* STAGE_NAMES[ST_COUNT] = {"trace_gen", "trace_ntt", "trace_merkle", "aux_columns", "aux_ntt", "aux_merkle",
                                            "quotient", "quotient_commit", "openings", "fri", "total"};

struct bn254s_proof {
  std::vector<u64> words, outputs;
  size_t sec_off[BN254S_SEC_COUNT + 1] = {0};  // bn254s_proof_section: start of every field of the word layout
  int degree_bits = 0;
  float stage_ms[ST_COUNT] = {0};
};

std::vector<int> fri_arities(const bn254s_params& P, int degree_bits) {  // ConstantArityBits(arity, final)
  std::vector<int> a;
  int d = degree_bits;
  while (d > (int)P.final_poly_bits && d + (int)P.rate_bits - (int)P.arity_bits >= (int)P.cap_height) {
    a.push_back(P.arity_bits);
    d -= P.arity_bits;
  }
  return a;
}

__global__ __launch_bounds__(256) void k_quotient_chunks(const u64* __restrict__ ab, u64* __restrict__ out, size_t N, u64 inv2,
                                                         u64 inv2c) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  int a = blockIdx.y;
  u64 A = ab[(size_t)(a * 2 + 0) * N + i], B = ab[(size_t)(a * 2 + 1) * N + i];
  out[(size_t)(a * 2 + 0) * N + i] = gl_mul(gl_add(A, B), inv2);
  out[(size_t)(a * 2 + 1) * N + i] = gl_mul(gl_sub(A, B), inv2c);
}

#define CHK(call)                                              \
  do {                                                         \
    hipError_t e_ = (call);                                    \
    if (e_ != hipSuccess) {                                    \
      err = std::string(#call) + ": " + hipGetErrorString(e_); \
      return BN254S_E_HIP;                                     \
    }                                                          \
  } while (0)

// Holds the context's big-kernel lock; on release waits until the slot's stream has drained.
struct BigSection {
  bn254s_ctx* c;
  hipStream_t st;
  int cls;
  BigSection(bn254s_ctx* c_, hipStream_t st_, int cls_) : c(c_), st(st_), cls(cls_) { c->big_lock(cls); }
  ~BigSection() {
    hipStreamSynchronize(st);
    c->big_unlock(cls);
  }
};

// Point tables are per degree; built once per context (bn254s_ctx_create thread or first prove call).
static int get_point_tables(bn254s_ctx* c, unsigned log_n, QPointTables& pt) {
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  std::string key = "pt." + std::to_string(log_n);
  bool fresh = !c->has(key);
  size_t M2 = (size_t)2 << log_n;
  u64* p = c->words(key, 3 * M2);
  if (!p) return BN254S_E_OOM;
  if (fresh) {
    quotient_point_tables(p, p + M2, p + 2 * M2, log_n, c->stream);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return BN254S_E_HIP;
  }
  pt.x = p;
  pt.lfirst = p + M2;
  pt.llast = p + 2 * M2;
  return 0;
}

// ---- workspace --------------------------------------------------------------------------------------------------
// The device memory of one proof: the named buffers of the slot (sizes: ProofPlan::words) and the pointers carved out of them.
struct Workspace {
  Slot* sl = nullptr;
  const ProofPlan* pl = nullptr;
  u64 *in, *tvals, *tcoef, *hist, *tmp, *ldechunk, *sponge, *comb, *tlde, *trees, *avals, *acoef, *alde, *scr, *quot, *tabs, *open,
      *fri, *fritrees, *qout;
  int* err;                 // device error word (behind the inputs)
  unsigned long long* pow;  // proof-of-work result
  u32* qidx;                // query indices (behind the query rounds)
  u64 *ttree, *atree, *qtree;
  u64 *qv, *ab, *qcoef, *qlde, *qpart;  // [2][2][N], [2][2][N], [4][N], [4][2N], [parts][2][2N]
  u64 *W, *mzt, *apow;
  size_t cap_off;  // of the cap inside a commitment tree
  // streaming workspace, from begin_windows() on: trace / auxiliary rows of a quotient window, its point tables, query leaf rows
  u64 *tw = nullptr, *aw = nullptr, *wpt = nullptr, *qrows = nullptr;
  int begin_windows(std::string& err);
};

// Buffer names, sizes and the order of drops and allocations are part of the behaviour: slots carry buffers from one proof to the
// next across workspace layouts, and the out-of-memory retry of the batch entry points depends on what is given back and when.
static int workspace_acquire(Slot& sl, const ProofPlan& pl, Workspace& ws, std::string& err) {
  BufPool& mem = sl.mem;
  const PlanBuffers& b = pl.words;
  const bool stream = pl.stream, lowmem = pl.lowmem;
  ws.sl = &sl;
  ws.pl = &pl;
  if (lowmem) {  // buffers of the plain layout left in the slot by an earlier, smaller proof would not fit beside this one
    mem.drop("acoef");
    mem.drop("alde");
  }
  ws.in = mem.words("in", b.in);
  ws.tvals = mem.words("tvals", b.tvals);
  ws.tcoef = mem.words("tcoef", b.tcoef);
  ws.hist = mem.words("hist", b.hist);
  ws.tmp = mem.words("tmp", b.tmp);
  mem.drop("win");  // (allocated in the middle of a streaming proof, in the memory of its dead trace values)
  if (stream) {  // no resident LDE: whatever an earlier proof left in the slot under these names goes first
    mem.drop("tlde");
    mem.drop("alde");
    mem.drop("acoef");
  } else {
    mem.drop("ldechunk");
    mem.drop("sponge");
  }
  ws.ldechunk = stream ? mem.words("ldechunk", b.ldechunk) : nullptr;
  ws.sponge = stream ? mem.words("sponge", b.sponge) : nullptr;
  ws.comb = mem.words("comb", b.comb);
  ws.tlde = stream ? ws.ldechunk : mem.words("tlde", b.tlde);
  ws.trees = mem.words("trees", b.trees);
  ws.avals = mem.words("avals", b.avals);
  ws.acoef = lowmem ? ws.avals : mem.words("acoef", b.acoef);  // compact workspace: the commitment runs in place
  ws.alde = stream ? ws.ldechunk : lowmem ? ws.tvals : mem.words("alde", b.alde);
  ws.scr = mem.words("scratch", b.scratch);
  ws.quot = mem.words("quot", b.quot);
  ws.tabs = mem.words("tabs", b.tabs);
  ws.open = mem.words("open", b.open);
  ws.fri = mem.words("fri", b.fri);
  ws.fritrees = mem.words("fritrees", b.fritrees);
  ws.qout = mem.words("qout", b.qout);
  // pinned staging for the two larger device -> host copies (opening partials, query rounds), part of the workspace
  if (sl.pinned_bytes < pl.pinned_bytes) {
    if (sl.pinned) hipHostFree(sl.pinned);
    sl.pinned = nullptr;
    sl.pinned_bytes = 0;
    CHK(hipHostMalloc(&sl.pinned, pl.pinned_bytes));
    sl.pinned_bytes = pl.pinned_bytes;
  }
  if (!ws.hist || !ws.in || !ws.tvals || !ws.tcoef || !ws.tmp || !ws.tlde || !ws.trees || !ws.avals || !ws.acoef || !ws.alde ||
      !ws.scr || !ws.quot || !ws.tabs || !ws.open || !ws.fri || !ws.fritrees || !ws.qout || !ws.comb ||
      (stream && (!ws.ldechunk || !ws.sponge))) {
    err = mem.err;
    mem.release();  // a workspace that could not be completed is given back: the context stays usable for smaller proofs
    return BN254S_E_OOM;
  }
  {
    // The HIP runtime allocates device memory of its own while kernels run (scratch for the kernels that spill, per hardware
    // queue; signals, kernel arguments): when that fails the queue aborts the whole process (HSA_STATUS_ERROR_OUT_OF_RESOURCES).
    // A workspace that leaves less than the reserve free is therefore given back and reported as out of memory, which the batch
    // entry points turn into "wait for a running proof to finish".  BN254S_MEM_RESERVE_MB overrides (default 6144).
    static const size_t reserve = (size_t)(getenv("BN254S_MEM_RESERVE_MB") ? atol(getenv("BN254S_MEM_RESERVE_MB")) : 6144) << 20;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b < reserve) {
      err = "device memory: " + std::to_string(free_b >> 20) + " MB would be left free, below the reserve of " +
            std::to_string(reserve >> 20) + " MB kept for the runtime's own allocations";
      mem.release();
      return BN254S_E_OOM;
    }
  }
  const size_t N = pl.N, M2 = pl.M2;
  const int NQ = ProofPlan::NQ;
  ws.err = (int*)(ws.in + pl.in_words);
  ws.pow = (unsigned long long*)(ws.in + pl.in_words + 2);
  ws.qidx = (u32*)(ws.qout + pl.n_q());
  ws.ttree = ws.trees;
  ws.atree = ws.trees + pl.tree_words;
  ws.qtree = ws.trees + 2 * pl.tree_words;
  ws.qv = ws.quot;
  ws.ab = ws.quot + (size_t)NQ * N;
  ws.qcoef = ws.quot + (size_t)2 * NQ * N;
  ws.qlde = ws.quot + (size_t)3 * NQ * N;
  ws.qpart = ws.qlde + (size_t)NQ * M2;
  ws.W = ws.tabs;
  ws.mzt = ws.tabs + QUOTIENT_W_WORDS(pl.K);
  ws.apow = ws.mzt + QUOTIENT_MZT_WORDS;
  ws.cap_off = 4 * merkle_level_offset(pl.log_m2, pl.log_m2 - pl.P.cap_height);
  return BN254S_OK;
}

// Streaming workspace, once the auxiliary values exist: the trace values are dead, their memory becomes the quotient windows (all
// columns x WROWS rows), the window's point tables and the leaf rows of the queries.
int Workspace::begin_windows(std::string& err) {
  BufPool& mem = sl->mem;
  const size_t WROWS = pl->WROWS;
  CHK(hipStreamSynchronize(sl->st));
  mem.drop("tvals");
  tvals = nullptr;
  u64* win = mem.words("win", pl->words.win);
  if (!win) {
    err = mem.err;
    mem.release();
    return BN254S_E_OOM;
  }
  tw = win;
  aw = win + (size_t)pl->W * WROWS;
  wpt = aw + (size_t)pl->A * WROWS;
  qrows = wpt + 3 * WROWS;
  return BN254S_OK;
}

// ---- stages -----------------------------------------------------------------------------------------------------
// What every stage of one proof works with.
struct Run {
  bn254s_ctx* c;
  Slot& sl;
  hipStream_t st;
  const ProofPlan& pl;
  Workspace& ws;
  const Transforms& tf;
  QPointTables pt;
  // one begin/end event pair per stage (they belong to the slot); a stage's time never includes waiting for the big-kernel lock
  void sb(int stage) const { hipEventRecord(sl.events[2 * stage], st); }
  void se(int stage) const { hipEventRecord(sl.events[2 * stage + 1], st); }
  // proofs running beside this one right now: the small Merkle levels use their throughput kernels then (merkle.h; same digests)
  int mmode() const { return c->workers.in_flight.load(std::memory_order_relaxed) >= 4 ? MERKLE_THROUGHPUT : MERKLE_LATENCY; }
};

// Uploads the job arrays to d_in = [scalars | x | offsets] and launches the kind's trace generator (shared by the trace stage and
// bn254s_generate_trace, which differ in stream, scratch owner and with_range).
static int upload_and_generate(const StarkKind& sk, const u64* scalars, const u64* x, const u64* off, size_t n, u64* d_in, u64* d_trace,
                               size_t N, u64* d_scr, u64* d_outs, int* d_err, hipStream_t st, bool with_range, std::string& err) {
  const size_t PW = sk.point_words;
  u64* d_sc = d_in;
  u64* d_x = d_in + 4 * n;
  u64* d_off = d_x + PW * n;
  CHK(hipMemcpyAsync(d_sc, scalars, n * 32, hipMemcpyHostToDevice, st));
  CHK(hipMemcpyAsync(d_x, x, n * PW * 8, hipMemcpyHostToDevice, st));
  if (sk.has_offset) CHK(hipMemcpyAsync(d_off, off, n * PW * 8, hipMemcpyHostToDevice, st));
  if (sk.generate_trace(d_sc, d_x, d_off, n, d_trace, N, d_scr, d_outs, d_err, st, with_range)) {
    err = "trace generation launch failed";
    return BN254S_E_HIP;
  }
  return BN254S_OK;
}

// trace generation (scalar_mul_stark.rs:55-69); *h_err is valid after the next synchronisation of the stream
static int stage_trace(const Run& r, const u64* scalars, const u64* x, const u64* off, bn254s_proof* pr, int* h_err, std::string& err) {
  const ProofPlan& pl = r.pl;
  const Workspace& ws = r.ws;
  const StarkShape& sh = pl.sh;
  hipStream_t st = r.st;
  r.sb(ST_TRACE);
  CHK(hipMemsetAsync(ws.err, 0, 16, st));
  u64* d_outs = ws.open;  // n*PW words fit (reused later)
  if (int rc = upload_and_generate(stark_kind(pl.kind), scalars, x, off, pl.n, ws.in, ws.tvals, pl.N, ws.scr, d_outs, ws.err, st, false, err))
    return rc;
  {
    // generate_range_checks: the histogram keeps 128 KB of LDS per workgroup on every CU, which would lock another proof's
    // NTT tiles (35 KB each) out of the CUs it shares: it takes its turn like the other wide kernels
    BigSection big(r.c, st, BIG_EXCL);
    launch_range_columns(ws.tvals, pl.N, sh.rc_begin, sh.rc_end, sh.freq_col, sh.table_col, (u32*)ws.hist, ws.err, st);
  }
  pr->outputs.resize(pl.n * (size_t)pl.PW);
  CHK(hipMemcpyAsync(pr->outputs.data(), d_outs, pl.n * (size_t)pl.PW * 8, hipMemcpyDeviceToHost, st));
  CHK(hipMemcpyAsync(h_err, ws.err, 4, hipMemcpyDeviceToHost, st));
  r.se(ST_TRACE);
  return BN254S_OK;
}

// leaf hash of a resident commitment: one GPU-filling section, or (BN254S_HASH_SPLIT, 2^16-row proofs) several shorter ones
static void hash_sections(const Run& r, const u64* lde, int width, u64* tree, int stage) {
  bn254s_ctx* c = r.c;
  const size_t M2 = r.pl.M2;
  const int S = r.pl.log_n == 16 ? c->hash_split : 1;
  if (S <= 1) {
    BigSection big(c, r.st, BIG_HASH);
    r.sb(stage);  // (the stage's clock starts once the section is admitted)
    merkle_leaves(lde, 1, M2, width, r.pl.log_m2, tree, r.st);
    return;
  }
  const size_t cnt = M2 / S;
  for (int k = 0; k < S; k++) {
    BigSection big(c, r.st, BIG_HASH_PART);
    if (k == 0) r.sb(stage);
    merkle_leaves_range(lde, 1, M2, width, (size_t)k * cnt, cnt, tree, r.st);
  }
}

// PolynomialBatch::from_values of `width` columns (prover.rs:31-38): coefficients, LDE, Merkle tree; the cap lands in cap_out
// (valid on return).  Streaming workspace: no LDE is kept (`lde` is unused), the NTT and the leaf hash alternate chunk by chunk
// in one section, timed as the NTT stage.
static int commit(const Run& r, const u64* vals, u64* coef, u64* lde, int width, u64* tree, int ntt_stage, int merkle_stage,
                  u64* cap_out, std::string& err) {
  const ProofPlan& pl = r.pl;
  hipStream_t st = r.st;
  if (pl.stream) {
    BigSection big(r.c, st, BIG_NTT);
    r.sb(ntt_stage);
    r.tf.commit_stream(vals, coef, width, tree);
    r.se(ntt_stage);
    r.sb(merkle_stage);
  } else {
    {
      BigSection big(r.c, st, BIG_NTT);
      r.sb(ntt_stage);
      r.tf.commit_ntt(vals, coef, lde, width);
      r.se(ntt_stage);
    }
    hash_sections(r, lde, width, tree, merkle_stage);
  }
  merkle_upper(pl.log_m2, pl.P.cap_height, tree, st, r.mmode());
  CHK(hipMemcpyAsync(cap_out, tree + r.ws.cap_off, ProofPlan::CAPW * 8, hipMemcpyDeviceToHost, st));
  r.se(merkle_stage);
  CHK(hipStreamSynchronize(st));
  return BN254S_OK;
}

// auxiliary columns: LogUp helpers and running sums, CTL running sums
static void stage_aux(const Run& r, const u64 betas[2], const u64 gammas[2]) {
  BigSection big(r.c, r.st, BIG_EXCL);
  r.sb(ST_AUX);
  aux_build(r.pl.sh, r.ws.tvals, r.pl.N, betas, gammas, r.ws.avals, r.ws.scr, r.ws.err, r.st);
  r.se(ST_AUX);
}

// Streaming workspace: the quotient values per coset and window of BK consecutive rows: the LDE of every column chunk is
// recomputed and the window's rows (plus the next one) are taken out in natural order; the quotient kernels then run on the window
// (QArgs window mode).
static void quotient_over_windows(const Run& r, const u64 betas[2], const u64 gammas[2]) {
  const ProofPlan& pl = r.pl;
  const Workspace& ws = r.ws;
  hipStream_t st = r.st;
  const size_t N = pl.N, M2 = pl.M2, BK = pl.BK, WROWS = pl.WROWS;
  BigSection big(r.c, st, BIG_NTT);
  r.sb(ST_QUOTIENT);
  QPointTables wpt;
  wpt.x = ws.wpt;
  wpt.lfirst = ws.wpt + WROWS;
  wpt.llast = ws.wpt + 2 * WROWS;
  for (int h = 0; h < 2; h++)
    for (size_t k0 = 0; k0 < N; k0 += BK) {
      r.tf.for_lde_chunks(ws.tcoef, pl.W, 1 << h, [&](int c0, int cn) {
        fri_extract_window(ws.ldechunk, M2, pl.log_n, h, k0, WROWS, cn, ws.tw + (size_t)c0 * WROWS, st);
      });
      r.tf.for_lde_chunks(ws.acoef, pl.A, 1 << h, [&](int c0, int cn) {
        fri_extract_window(ws.ldechunk, M2, pl.log_n, h, k0, WROWS, cn, ws.aw + (size_t)c0 * WROWS, st);
      });
      quotient_point_tables_window(ws.wpt, ws.wpt + WROWS, ws.wpt + 2 * WROWS, pl.log_n, h, k0, WROWS, st);
      QArgs QA;
      quotient_fill_args(QA, pl.sh, nullptr, nullptr, ws.W, ws.mzt, r.pt, betas, gammas, pl.log_n, ws.qv, ws.qpart);
      quotient_window_args(QA, ws.tw, ws.aw, wpt, ws.qpart, WROWS, BK, k0, h);
      stark_kind(pl.kind).quotient_launch(QA, pl.sh, st);
    }
}

// quotient values on both cosets, their four chunk polynomials, and the quotient commitment; the cap lands in cap_out
static int stage_quotient(const Run& r, const u64 alphas[2], const u64 betas[2], const u64 gammas[2], u64* cap_out, std::string& err) {
  const ProofPlan& pl = r.pl;
  const Workspace& ws = r.ws;
  const StarkKind& sk = stark_kind(pl.kind);
  hipStream_t st = r.st;
  const size_t N = pl.N;
  {
    std::vector<u64> hW, hmzt;
    const int* mz_e0 = nullptr;
    const int nblk = sk.mz_blocks(&mz_e0);
    quotient_host_tables(pl.K, alphas, mz_e0, nblk, hW, hmzt);
    CHK(hipMemcpyAsync(ws.W, hW.data(), hW.size() * 8, hipMemcpyHostToDevice, st));
    CHK(hipMemcpyAsync(ws.mzt, hmzt.data(), hmzt.size() * 8, hipMemcpyHostToDevice, st));
    CHK(hipStreamSynchronize(st));  // host vectors go out of scope
  }
  if (pl.stream) {
    quotient_over_windows(r, betas, gammas);
  } else {
    BigSection big(r.c, st, BIG_EXCL);
    r.sb(ST_QUOTIENT);
    QArgs QA;
    quotient_fill_args(QA, pl.sh, ws.tlde, ws.alde, ws.W, ws.mzt, r.pt, betas, gammas, pl.log_n, ws.qv, ws.qpart);
    sk.quotient_launch(QA, pl.sh, st);
  }
  r.tf.quotient_coset_inverse(ws.qv, ws.ab);
  {
    u64 gn = gl_pow(GL_GEN, N);
    u64 inv2 = gl_inv(2), inv2c = gl_inv(gl_mul(2, gn));
    dim3 g((unsigned)((N + 255) / 256), 2);
    k_quotient_chunks<<<g, 256, 0, st>>>(ws.ab, ws.qcoef, N, inv2, inv2c);
  }
  r.se(ST_QUOTIENT);
  r.sb(ST_QUOTIENT_COMMIT);
  r.tf.lde(ws.qcoef, ws.qlde, ProofPlan::NQ);
  merkle_build(ws.qlde, 1, pl.M2, ProofPlan::NQ, pl.log_m2, pl.P.cap_height, ws.qtree, st, r.mmode());
  CHK(hipMemcpyAsync(cap_out, ws.qtree + ws.cap_off, ProofPlan::CAPW * 8, hipMemcpyDeviceToHost, st));
  r.se(ST_QUOTIENT_COMMIT);
  CHK(hipStreamSynchronize(st));
  return BN254S_OK;
}

// openings on the device (StarkOpeningSet::new): partial evaluations per polynomial and block, copied to h_part (valid on return)
static int stage_openings(const Run& r, gl2 zeta, gl2 zeta_next, u64* h_part, std::string& err) {
  const ProofPlan& pl = r.pl;
  const Workspace& ws = r.ws;
  hipStream_t st = r.st;
  const int W = pl.W, A = pl.A, NQ = ProofPlan::NQ, NSPL = pl.NSPL;
  const size_t R = pl.R, NH = pl.NH;
  {
    BigSection big(r.c, st, BIG_EXCL);
    r.sb(ST_OPENINGS);
    // split level: P(z) = Pe(z^2) + z Po(z^2), the halves are polynomials of NH coefficients opened at z^2 and (g z)^2
    u64* d_otab = ws.open + pl.n_part();
    fri_opening_tables(pl.log_r, pl.log_s ? gl2_mul(zeta, zeta) : zeta, pl.log_s ? gl2_mul(zeta_next, zeta_next) : zeta_next, d_otab, st);
    fri_openings(ws.tcoef, NH, pl.log_r, W * NSPL, d_otab, ws.open, st);
    fri_openings(ws.acoef, NH, pl.log_r, A * NSPL, d_otab, ws.open + (size_t)W * NSPL * R * 5, st);
    fri_openings(ws.qcoef, NH, pl.log_r, NQ * NSPL, d_otab, ws.open + (size_t)(W + A) * NSPL * R * 5, st);
  }
  CHK(hipMemcpyAsync(h_part, ws.open, pl.n_part() * 8, hipMemcpyDeviceToHost, st));
  r.se(ST_OPENINGS);
  CHK(hipStreamSynchronize(st));
  return BN254S_OK;
}

// Recombination of the opening partials: P(z) = sum_k1 z^k1 S_k1(z^R) (transposed coefficient layout); P(1) = sum of the block
// sums.  h_open[p] = {P(zeta).c0, .c1, P(g zeta).c0, .c1, P(1)} for p over (trace | auxiliary | quotient chunks).
static std::vector<u64> recombine_openings(const ProofPlan& pl, const u64* h_part, gl2 zeta, gl2 zeta_next) {
  const size_t R = pl.R;
  const int NSPL = pl.NSPL, n_polys = pl.W + pl.A + ProofPlan::NQ;
  std::vector<u64> h_open((size_t)n_polys * 5);
  std::vector<gl2> zp0(R), zp1(R);
  gl2 a = gl2_make(1, 0), b = gl2_make(1, 0);
  const gl2 y0 = pl.log_s ? gl2_mul(zeta, zeta) : zeta, y1 = pl.log_s ? gl2_mul(zeta_next, zeta_next) : zeta_next;
  for (size_t k1 = 0; k1 < R; k1++) {
    zp0[k1] = a;
    zp1[k1] = b;
    a = gl2_mul(a, y0);
    b = gl2_mul(b, y1);
  }
  for (int p = 0; p < n_polys; p++) {
    gl2 v0 = gl2_make(0, 0), v1 = gl2_make(0, 0);
    u64 s1 = 0;
    for (int half = 0; half < NSPL; half++) {
      gl2 e0 = gl2_make(0, 0), e1 = gl2_make(0, 0);
      for (size_t k1 = 0; k1 < R; k1++) {
        const u64* q = &h_part[(((size_t)p * NSPL + half) * R + k1) * 5];
        e0 = gl2_add(e0, gl2_mul(zp0[k1], gl2_make(q[0], q[1])));
        e1 = gl2_add(e1, gl2_mul(zp1[k1], gl2_make(q[2], q[3])));
        s1 = gl_add(s1, q[4]);
      }
      v0 = gl2_add(v0, half ? gl2_mul(zeta, e0) : e0);
      v1 = gl2_add(v1, half ? gl2_mul(zeta_next, e1) : e1);
    }
    u64* o5 = &h_open[(size_t)p * 5];
    o5[0] = v0.c0; o5[1] = v0.c1; o5[2] = v1.c0; o5[3] = v1.c1; o5[4] = s1;
  }
  return h_open;
}

// The opening set as the transcript and the proof see it: value k of polynomial p of h_open, and where the CTL running sums sit.
struct Openings {
  const ProofPlan& pl;
  const std::vector<u64>& h_open;
  u64 operator()(int p, int k) const { return h_open[(size_t)p * 5 + k]; }
  int n_ctlz() const { return 2 * pl.sh.n_ctl; }
  u64 ctl_z_first(int i) const { return (*this)(pl.W + pl.sh.n_lookup_cols() + i, 4); }
};

// to_fri_openings order: (local | aux | quotient) at zeta, (next | aux_next) at g*zeta, ctl_zs_first
static void observe_openings(Challenger& ch, const Openings& op) {
  const int W = op.pl.W, A = op.pl.A, NQ = ProofPlan::NQ;
  for (int p = 0; p < W + A + NQ; p++) {
    ch.observe(op(p, 0));
    ch.observe(op(p, 1));
  }
  for (int p = 0; p < W + A; p++) {
    ch.observe(op(p, 2));
    ch.observe(op(p, 3));
  }
  for (int i = 0; i < op.n_ctlz(); i++) {
    ch.observe(op.ctl_z_first(i));
    ch.observe(0);
  }
}

// The powers of the FRI batching challenge: alpha^p cut in 22-bit limbs (quotient_common.h W3), 8 u32 per power, for the device;
// and the alpha-weighted sums of the openings of the three batches (at zeta, at g zeta, at 1).
struct FriAlphaPowers {
  std::vector<u32> apow;
  gl2 r0, r1, r2;
};
static FriAlphaPowers fri_alpha_powers(const Openings& op, gl2 fri_alpha) {
  const int W = op.pl.W, A = op.pl.A, NQ = ProofPlan::NQ, n_ctlz = op.n_ctlz();
  FriAlphaPowers f;
  f.apow.assign(8 * (size_t)(W + A + NQ), 0);
  gl2 ap = gl2_make(1, 0);
  f.r0 = f.r1 = f.r2 = gl2_make(0, 0);
  for (int p = 0; p < W + A + NQ; p++) {
    fri_weight_record(&f.apow[8 * (size_t)p], ap);
    f.r0 = gl2_add(f.r0, gl2_mul(ap, gl2_make(op(p, 0), op(p, 1))));
    if (p < W + A) f.r1 = gl2_add(f.r1, gl2_mul(ap, gl2_make(op(p, 2), op(p, 3))));
    if (p < n_ctlz) f.r2 = gl2_add(f.r2, gl2_mul_base(ap, op.ctl_z_first(p)));
    ap = gl2_mul(ap, fri_alpha);
  }
  return f;
}

// FRI batch polynomial on the LDE domain (prove_openings -> the first layer's values in ws.fri)
static int stage_fri_combine(const Run& r, const FriAlphaPowers& f, gl2 zeta, gl2 zeta_next, gl2 fri_alpha, std::string& err) {
  const ProofPlan& pl = r.pl;
  const Workspace& ws = r.ws;
  hipStream_t st = r.st;
  CHK(hipMemcpyAsync(ws.apow, f.apow.data(), f.apow.size() * 4, hipMemcpyHostToDevice, st));
  CHK(hipStreamSynchronize(st));
  BigSection big(r.c, st, BIG_EXCL);
  r.sb(ST_FRI);
  // The batch polynomial is linear in the committed polynomials: its three alpha-weighted sums are formed on the coefficient
  // vectors (N points, not the 2N of the LDE; in the compact workspace acoef is avals, still live: the openings above read
  // it), then one LDE of the six sum columns, then the point-wise part.  The same field elements as summing the LDE values.
  fri_combine_coeffs(pl.sh, ws.tcoef, ws.acoef, ws.qcoef, ws.apow, pl.N, ws.comb, st);
  r.tf.lde(ws.comb, ws.comb + (size_t)6 * pl.N, 6);
  fri_combine_final(pl.sh, ws.comb + (size_t)6 * pl.N, r.pt.x, zeta, zeta_next, f.r0, f.r1, f.r2, fri_alpha, pl.M2, ws.fri, st);
  return BN254S_OK;
}

// The committed FRI layers, and what is left after the last fold.
struct FriLayers {
  std::vector<std::vector<u64>> caps;
  std::vector<const u64*> vals, trees;
  const u64* last = nullptr;  // values of the final layer: 2^lm extension elements on the coset shift * <w>, bit-reversed
  u64 shift = GL_GEN;
  unsigned lm = 0;
};

// FRI commit phase: per layer the Merkle tree of the 16-element cosets, its cap into the transcript, the fold by the challenge
static int stage_fri_commit(const Run& r, Challenger& ch, FriLayers& fl, std::string& err) {
  const ProofPlan& pl = r.pl;
  hipStream_t st = r.st;
  const int L = pl.L, CAPW = ProofPlan::CAPW;
  fl.caps.assign(L, std::vector<u64>(CAPW));
  fl.vals.resize(L);
  fl.trees.resize(L);
  u64* vals = r.ws.fri;
  u64* ftree = r.ws.fritrees;
  fl.shift = GL_GEN;
  unsigned lm = pl.log_m2;
  const u64 inv16 = gl_inv(16);
  for (int l = 0; l < L; l++) {
    const int lg = (int)lm - 4;
    merkle_build(vals, 32, 1, 32, lg, pl.P.cap_height, ftree, st, r.mmode());
    CHK(hipMemcpyAsync(fl.caps[l].data(), ftree + 4 * merkle_level_offset(lg, lg - pl.P.cap_height), CAPW * 8,
                       hipMemcpyDeviceToHost, st));
    CHK(hipStreamSynchronize(st));
    ch.observe_n(fl.caps[l].data(), CAPW);
    gl2 beta = ch.challenge_ext();
    u64* next = vals + 2 * ((size_t)1 << lm);
    fri_fold(vals, next, lm, fl.shift, beta, inv16, st);
    fl.vals[l] = vals;
    fl.trees[l] = ftree;
    ftree += merkle_tree_digests(lg, pl.P.cap_height) * 4;
    vals = next;
    fl.shift = gl_pow(fl.shift, 16);
    lm -= 4;
  }
  fl.last = vals;
  fl.lm = lm;
  return BN254S_OK;
}

// final polynomial: coset iDFT of the last (tiny) layer on the host, upper half must vanish
static int fri_final_poly(const std::vector<u64>& h_final, unsigned lm, u64 shift, unsigned rate_bits, std::vector<gl2>& final_poly,
                          std::string& err) {
  const size_t Mf = (size_t)1 << lm;
  final_poly.assign(Mf >> rate_bits, gl2_make(0, 0));
  const u64 w = gl_root_of_unity(lm), winv = gl_inv(w), sinv = gl_inv(shift), minv = gl_inv((u64)Mf);
  for (size_t k = 0; k < Mf; k++) {
    gl2 acc = gl2_make(0, 0);
    u64 wk = gl_pow(winv, k), t = 1;
    for (size_t nn = 0; nn < Mf; nn++) {  // value at natural index nn sits at position bitrev(nn)
      size_t pos = bitrev32((u32)nn, lm);
      acc = gl2_add(acc, gl2_mul_base(gl2_make(h_final[2 * pos], h_final[2 * pos + 1]), t));
      t = gl_mul(t, wk);
    }
    acc = gl2_mul_base(acc, gl_mul(minv, gl_pow(sinv, k)));
    if (k < final_poly.size()) final_poly[k] = acc;
    else if (acc.c0 | acc.c1) {
      err = "FRI final polynomial has non-zero high coefficients";
      return BN254S_E_INTERNAL;
    }
  }
  return BN254S_OK;
}

// proof of work (fri_proof_of_work): smallest witness with >= pow_bits leading zeros in the response
static int stage_pow(const Run& r, Challenger& ch, u64& pow_witness, std::string& err) {
  const unsigned pow_bits = r.pl.P.pow_bits;
  hipStream_t st = r.st;
  u64 stt[12];
  memcpy(stt, ch.state, sizeof(stt));
  for (int i = 0; i < ch.in_len; i++) stt[i] = ch.in_buf[i];
  const size_t WIN = (size_t)1 << (pow_bits + 1);  // 86 % of the searches end in the first window
  unsigned long long found = ~0ULL;
  for (u64 base = 0; found == ~0ULL; base += WIN) {
    CHK(hipMemsetAsync(r.ws.pow, 0xFF, 8, st));
    fri_pow_launch(stt, ch.in_len, base, pow_bits, WIN, r.ws.pow, st);
    CHK(hipMemcpyAsync(&found, r.ws.pow, 8, hipMemcpyDeviceToHost, st));
    CHK(hipStreamSynchronize(st));
    if (base > ((u64)1 << 40)) {
      err = "proof of work not found";
      return BN254S_E_INTERNAL;
    }
  }
  pow_witness = found;
  ch.observe(pow_witness);
  u64 resp = ch.challenge();
  if (resp >> (64 - pow_bits)) {
    err = "proof of work self-check failed";
    return BN254S_E_INTERNAL;
  }
  return BN254S_OK;
}

// query rounds: the indices from the transcript, every opened row and Merkle path gathered on the device into h_q (valid on
// return); closes the FRI stage and the proof's clock, and reads the device error word
static int stage_queries(const Run& r, Challenger& ch, const FriLayers& fl, u64* h_q, std::string& err) {
  const ProofPlan& pl = r.pl;
  const Workspace& ws = r.ws;
  hipStream_t st = r.st;
  const int W = pl.W, A = pl.A, L = pl.L, nq = (int)pl.P.num_queries;
  std::vector<u32> qidx(pl.P.num_queries);
  for (auto& q : qidx) q = (u32)(ch.challenge() % pl.M2);
  CHK(hipMemcpyAsync(ws.qidx, qidx.data(), qidx.size() * 4, hipMemcpyHostToDevice, st));
  if (pl.stream) {  // leaf rows of the queries: one more pass of chunk LDEs, 84 rows taken out of each
    r.tf.for_lde_chunks(ws.tcoef, W, 3, [&](int c0, int cn) {
      fri_gather_rows(ws.ldechunk, pl.M2, cn, ws.qidx, nq, ws.qrows + (size_t)c0 * nq, st);
    });
    r.tf.for_lde_chunks(ws.acoef, A, 3, [&](int c0, int cn) {
      fri_gather_rows(ws.ldechunk, pl.M2, cn, ws.qidx, nq, ws.qrows + (size_t)(W + c0) * nq, st);
    });
  }
  {
    QueryGatherArgs G;
    G.lde[0] = ws.tlde; G.lde[1] = ws.alde; G.lde[2] = ws.qlde;
    if (pl.stream) {
      G.lde[0] = ws.qrows;
      G.lde[1] = ws.qrows + (size_t)W * pl.P.num_queries;
      G.lde_by_query[0] = G.lde_by_query[1] = 1;
    }
    G.tree[0] = ws.ttree; G.tree[1] = ws.atree; G.tree[2] = ws.qtree;
    G.width[0] = W; G.width[1] = A; G.width[2] = ProofPlan::NQ;
    for (int l = 0; l < L; l++) {
      G.layer_vals[l] = fl.vals[l];
      G.layer_tree[l] = fl.trees[l];
    }
    G.n_layers = L;
    G.log_m2 = pl.log_m2;
    G.cap_height = pl.P.cap_height;
    G.M2 = pl.M2;
    G.indices = ws.qidx;
    G.out = ws.qout;
    G.words_per_query = pl.wpq;
    fri_gather_queries(G, pl.P.num_queries, st);
  }
  int h_err = 0;
  CHK(hipMemcpyAsync(h_q, ws.qout, pl.n_q() * 8, hipMemcpyDeviceToHost, st));
  CHK(hipMemcpyAsync(&h_err, ws.err, 4, hipMemcpyDeviceToHost, st));
  r.se(ST_FRI);
  r.se(ST_TOTAL);
  CHK(hipStreamSynchronize(st));
  CHK(hipGetLastError());
  if (h_err) {
    err = "device self-check failed: " + std::to_string(h_err);
    return h_err;
  }
  return BN254S_OK;
}

// What the host holds of a proof before its words are laid out.
struct ProofParts {
  u64 caps[3][64];  // trace, auxiliary, quotient
  u64 init_state[12];
  std::vector<u64> h_open;
  FriLayers fri;
  std::vector<gl2> final_poly;
  u64 pow_witness = 0;
  const u64* h_q = nullptr;  // query rounds (pinned staging)
};

// assemble (layout: include/bn254_stark.h)
static void assemble_proof(const ProofPlan& pl, const ProofParts& pp, bn254s_proof* pr) {
  const int W = pl.W, A = pl.A, NQ = ProofPlan::NQ, CAPW = ProofPlan::CAPW, L = pl.L;
  const Openings op{pl, pp.h_open};
  const int n_ctlz = op.n_ctlz();
  std::vector<u64>& o = pr->words;
  o.clear();
  o.reserve(3 * CAPW + 4 * (W + A) + n_ctlz + 2 * NQ + L * CAPW + pl.n_q() + 2 * pp.final_poly.size() + 13);
  auto mark = [&](int id) { pr->sec_off[id] = o.size(); };
  for (int t = 0; t < 3; t++) { mark(BN254S_SEC_TRACE_CAP + t); o.insert(o.end(), pp.caps[t], pp.caps[t] + CAPW); }
  mark(BN254S_SEC_LOCAL_VALUES);
  for (int p = 0; p < W; p++) { o.push_back(op(p, 0)); o.push_back(op(p, 1)); }
  mark(BN254S_SEC_NEXT_VALUES);
  for (int p = 0; p < W; p++) { o.push_back(op(p, 2)); o.push_back(op(p, 3)); }
  mark(BN254S_SEC_AUX_POLYS);
  for (int p = W; p < W + A; p++) { o.push_back(op(p, 0)); o.push_back(op(p, 1)); }
  mark(BN254S_SEC_AUX_POLYS_NEXT);
  for (int p = W; p < W + A; p++) { o.push_back(op(p, 2)); o.push_back(op(p, 3)); }
  mark(BN254S_SEC_CTL_ZS_FIRST);
  for (int i = 0; i < n_ctlz; i++) o.push_back(op.ctl_z_first(i));
  mark(BN254S_SEC_QUOTIENT_POLYS);
  for (int p = W + A; p < W + A + NQ; p++) { o.push_back(op(p, 0)); o.push_back(op(p, 1)); }
  mark(BN254S_SEC_FRI_CAPS);
  for (int l = 0; l < L; l++) o.insert(o.end(), pp.fri.caps[l].begin(), pp.fri.caps[l].end());
  mark(BN254S_SEC_QUERY_ROUNDS);
  o.insert(o.end(), pp.h_q, pp.h_q + pl.n_q());
  mark(BN254S_SEC_FINAL_POLY);
  for (auto& cf : pp.final_poly) { o.push_back(cf.c0); o.push_back(cf.c1); }
  mark(BN254S_SEC_POW_WITNESS);
  o.push_back(pp.pow_witness);
  mark(BN254S_SEC_INIT_CHALLENGER_STATE);
  o.insert(o.end(), pp.init_state, pp.init_state + 12);
  mark(BN254S_SEC_COUNT);
  pr->degree_bits = pl.log_n;
}

// One proof on a slot: the stages in the order of starks/common/prover.rs, the transcript between them.
// `after_alloc` (optional) is called once the workspace of the proof is complete: the out-of-memory retry of the batch entry
// points holds WorkPool::retry_mu up to that point, so that allocation attempts never interleave.
static int prove_on_slot(bn254s_ctx* c, Slot& sl, int kind, const bn254s_params& P, const u64* scalars, const u64* x,
                         const u64* off, size_t n, bn254s_proof* pr, std::string& err,
                         const std::function<void()>* after_alloc = nullptr) {
  // which workspace the proof gets depends on the device's memory; the test overrides are read per call
  size_t dev_free_b = 0, dev_total_b = 0;
  (void)hipMemGetInfo(&dev_free_b, &dev_total_b);
  ProofPlan pl;
  if (int rc = proof_plan(kind, n, P, dev_total_b, plan_overrides_from_env(), pl, err)) return rc;
  hipStream_t st = sl.st;
  QPointTables pt;
  if (int rc = get_point_tables(c, pl.log_n, pt)) {
    err = "point tables";
    return rc;
  }
  const NttPlan* np = c->ntt_plan(pl.log_n, pl.log_s != 0);
  if (!np) {
    err = "NTT tables";
    return BN254S_E_OOM;
  }
  Workspace ws;
  if (int rc = workspace_acquire(sl, pl, ws, err)) return rc;
  if (after_alloc) (*after_alloc)();
  const Transforms tf{*np, st, pl, ws.tmp, ws.ldechunk, ws.sponge};
  if (sl.events.empty()) {
    sl.events.resize(2 * ST_COUNT);
    for (auto& e : sl.events) CHK(hipEventCreate(&e));
  }
  const Run r{c, sl, st, pl, ws, tf, pt};
  const int CAPW = ProofPlan::CAPW;
  ProofParts pp;
  Challenger ch;

  // ---- trace and its commitment (prover.rs:31-38) -----------------------------------------------------------
  r.sb(ST_TOTAL);
  int h_err = 0;
  if (int rc = stage_trace(r, scalars, x, off, pr, &h_err, err)) return rc;
  if (int rc = commit(r, ws.tvals, ws.tcoef, ws.tlde, pl.W, ws.ttree, ST_TRACE_NTT, ST_TRACE_MERKLE, pp.caps[0], err)) return rc;
  if (h_err) {
    err = "trace generation reported device error " + std::to_string(h_err);
    return h_err;
  }
  // ---- transcript: trace cap, CTL challenges, compact (prover.rs:40-54) --------------------------------
  ch.observe_n(pp.caps[0], CAPW);
  u64 betas[2], gammas[2];
  for (int i = 0; i < 2; i++) {
    betas[i] = ch.challenge();
    gammas[i] = ch.challenge();
  }
  ch.compact(pp.init_state);

  // ---- auxiliary columns + commitment ---------------------------------------------------------------------
  stage_aux(r, betas, gammas);
  if (pl.stream)
    if (int rc = ws.begin_windows(err)) return rc;
  if (int rc = commit(r, ws.avals, ws.acoef, ws.alde, pl.A, ws.atree, ST_AUX_NTT, ST_AUX_MERKLE, pp.caps[1], err)) return rc;
  ch.observe_n(pp.caps[1], CAPW);
  u64 alphas[2] = {ch.challenge(), 0};
  alphas[1] = ch.challenge();

  // ---- quotient + commitment --------------------------------------------------------------------------------
  if (int rc = stage_quotient(r, alphas, betas, gammas, pp.caps[2], err)) return rc;
  ch.observe_n(pp.caps[2], CAPW);
  gl2 zeta = ch.challenge_ext();
  {
    gl2 zp = zeta;
    for (unsigned i = 0; i < pl.log_n; i++) zp = gl2_mul(zp, zp);
    if (gl2_eq(zp, gl2_make(1, 0))) {
      err = "Opening point is in the subgroup.";
      return BN254S_E_TRANSCRIPT;
    }
  }
  const gl2 zeta_next = gl2_mul_base(zeta, gl_root_of_unity(pl.log_n));

  // ---- openings (StarkOpeningSet::new) ---------------------------------------------------------------------
  // device -> host copies land in the slot's pinned staging buffer (pageable destinations go through a runtime-internal
  // staging allocation that costs ~8 ms the first time and an extra copy every time)
  u64* staging = (u64*)sl.pinned;
  if (int rc = stage_openings(r, zeta, zeta_next, staging, err)) return rc;
  pp.h_open = recombine_openings(pl, staging, zeta, zeta_next);
  const Openings op{pl, pp.h_open};
  observe_openings(ch, op);

  // ---- FRI (prove_openings) ------------------------------------------------------------------------------------
  const gl2 fri_alpha = ch.challenge_ext();
  if (int rc = stage_fri_combine(r, fri_alpha_powers(op, fri_alpha), zeta, zeta_next, fri_alpha, err)) return rc;
  if (int rc = stage_fri_commit(r, ch, pp.fri, err)) return rc;
  std::vector<u64> h_final((size_t)2 << pp.fri.lm);
  CHK(hipMemcpyAsync(h_final.data(), pp.fri.last, h_final.size() * 8, hipMemcpyDeviceToHost, st));
  CHK(hipStreamSynchronize(st));
  if (int rc = fri_final_poly(h_final, pp.fri.lm, pp.fri.shift, P.rate_bits, pp.final_poly, err)) return rc;
  for (auto& cf : pp.final_poly) {
    ch.observe(cf.c0);
    ch.observe(cf.c1);
  }
  if (int rc = stage_pow(r, ch, pp.pow_witness, err)) return rc;
  pp.h_q = staging;  // (the opening partials in it were consumed above)
  if (int rc = stage_queries(r, ch, pp.fri, staging, err)) return rc;

  assemble_proof(pl, pp, pr);
  for (int i = 0; i < ST_COUNT; i++) hipEventElapsedTime(&pr->stage_ms[i], sl.events[2 * i], sl.events[2 * i + 1]);
  return BN254S_OK;
}

// ---- C ABI ------------------------------------------------------------------------------------------------------
extern "C" {

// A batch in flight: proof i of the batch is one task of the context's worker pool (ctx.h WorkPool).
struct bn254s_batch {
  bn254s_ctx* c = nullptr;
  int kind = 0;
  bn254s_params params;
  const u64 *scalars = nullptr, *x = nullptr, *off = nullptr;
  size_t n_total = 0, per_proof = 0, n_proofs = 0;
  bn254s_proof** out = nullptr;
  std::mutex mu;
  std::condition_variable cv;
  size_t remaining = 0;
  int first_rc = 0;
  std::string err;
};

int bn254s_prove_batch_begin(bn254s_ctx* c, int kind, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x,
                             const uint64_t* off, size_t n_total, size_t per_proof, bn254s_proof** proofs_out,
                             bn254s_batch** handle) {
  if (!c || kind < 0 || kind > 2 || !params || !scalars || !x || (kind != KIND_FQ && !off) || !proofs_out || !handle || n_total == 0 ||
      per_proof == 0 || params->struct_size != sizeof(bn254s_params))
    return BN254S_E_INVALID_ARG;
  *handle = nullptr;
  const size_t n_proofs = (n_total + per_proof - 1) / per_proof;
  const size_t PW = stark_kind(kind).point_words;
  for (size_t i = 0; i < n_proofs; i++) proofs_out[i] = nullptr;
  HIP_TRY(c, hipSetDevice(c->device));
  // proofs in flight (one stream, host thread and workspace each; the streams share GPU_MAX_HW_QUEUES = 16 hardware queues - more
  // queues than that collapse the throughput: 24 / 32 queues gave 62 / 51 proofs/s).  Round 3, with arrival-order admission of the
  // wide sections: every queued proof should find a slot at once (32 proofs queued on 24 slots: 77.8 proofs/s; on 32 slots: 87.9),
  // and more proofs in flight keep a wide section ready at all times - bench.py with 8 / 16 / 24 / 32 proofs queued and as many
  // slots: 83.9 / 84.8 / 87.3 / 87.9 proofs/s (tools/gpu_depth_sweep.sh, gpu_depth_sweep2.sh); 48: 67.  A slot that is never used
  // costs a stream; its workspace (~4 GB for a 2^16-row proof) is allocated on first use.
  size_t n_slots = 32;
  if (const char* e = getenv("BN254S_SLOTS")) n_slots = std::min((size_t)bn254s_ctx::MAX_SLOTS, (size_t)std::max(1, atoi(e)));
  for (size_t s = 0; s < n_slots; s++)
    if (!c->slot(s)) return BN254S_E_HIP;
  c->workers.start(n_slots, c->device);
  bn254s_batch* B = new bn254s_batch();
  B->c = c;
  B->kind = kind;
  B->params = *params;
  B->scalars = scalars;
  B->x = x;
  B->off = off;
  B->n_total = n_total;
  B->per_proof = per_proof;
  B->n_proofs = n_proofs;
  B->out = proofs_out;
  B->remaining = n_proofs;
  for (size_t i = 0; i < n_proofs; i++)
    c->workers.push([B, i, PW](size_t s) {
      bool skip;
      {
        std::lock_guard<std::mutex> lk(B->mu);
        skip = B->first_rc != 0;  // an earlier proof of this batch failed: the call returns that error
      }
      if (!skip) {
        const size_t b = i * B->per_proof, cnt = std::min(B->per_proof, B->n_total - b);
        bn254s_proof* pr = new bn254s_proof();
        std::string err;
        bn254s_ctx* c = B->c;
        Slot& sl = *c->slot(s);
        auto attempt = [&](const std::function<void()>* after_alloc) {
          err.clear();
          return prove_on_slot(c, sl, B->kind, B->params, B->scalars + 4 * b, B->x + PW * b, B->off ? B->off + PW * b : nullptr, cnt,
                               pr, err, after_alloc);
        };
        int rc = attempt(nullptr);
        // Out of device memory: the workspaces the idle slots keep from earlier (smaller or differently shaped) proofs may be
        // what is in the way - give those back and try again; while other proofs are still running, wait for one of them to
        // finish and repeat (a batch of tall proofs then runs as many at a time as fit).  Alone and still too large: the error.
        // One task at a time does this (retry_mu, held until its workspace is complete or has been given back): two proofs
        // that both fit alone never fail on each other's partial workspaces, and "nobody else is running" is decided under
        // the same lock.  The completion counter is sampled before the attempt, so a proof that ends during it is not missed.
        WorkPool& wp = c->workers;
        while (rc == BN254S_E_OOM) {
          std::unique_lock<std::mutex> rl(wp.retry_mu);
          const size_t c0 = wp.completions_now();
          wp.for_idle_slots([&](size_t i) {
            if (i < c->n_slots_now()) c->slot(i)->mem.release();
          });
          const bool last = wp.active() <= 1;  // nobody else is running: nothing more will be given back
          const std::function<void()> unlock = [&]() { rl.unlock(); };
          rc = attempt(&unlock);
          if (rl.owns_lock()) rl.unlock();
          if (rc != BN254S_E_OOM || last) break;
          wp.wait_for_a_completion(c0);
        }
        if (rc != BN254S_OK) {
          hipStreamSynchronize(sl.st);
          delete pr;
          std::lock_guard<std::mutex> lk(B->mu);
          if (B->first_rc == 0) {
            B->first_rc = rc;
            B->err = err;
          }
        } else {
          B->out[i] = pr;
        }
      }
      std::lock_guard<std::mutex> lk(B->mu);  // (notify under the lock: the waiter frees the batch)
      if (--B->remaining == 0) B->cv.notify_all();
    });
  *handle = B;
  return BN254S_OK;
}

int bn254s_prove_batch_end(bn254s_batch* B) {
  if (!B) return BN254S_E_INVALID_ARG;
  {
    std::unique_lock<std::mutex> lk(B->mu);
    B->cv.wait(lk, [&] { return B->remaining == 0; });
  }
  const int rc = B->first_rc;
  if (rc) {
    B->c->set_err(B->err);
    for (size_t i = 0; i < B->n_proofs; i++) {
      delete B->out[i];
      B->out[i] = nullptr;
    }
  }
  delete B;
  return rc;
}

int bn254s_prove_batch(bn254s_ctx* c, int kind, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x,
                       const uint64_t* off, size_t n_total, size_t per_proof, bn254s_proof** proofs_out) {
  bn254s_batch* B = nullptr;
  int rc = bn254s_prove_batch_begin(c, kind, params, scalars, x, off, n_total, per_proof, proofs_out, &B);
  return rc != BN254S_OK ? rc : bn254s_prove_batch_end(B);
}

int bn254s_prove_g1_batch(bn254s_ctx* c, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x,
                          const uint64_t* off, size_t n_total, size_t per_proof, bn254s_proof** proofs_out) {
  return bn254s_prove_batch(c, KIND_G1, params, scalars, x, off, n_total, per_proof, proofs_out);
}

// The single-proof entry points queue ONE proof of n instances on the worker pool, like a batch of one: a call made while a
// batch is open (between bn254s_prove_batch_begin and _end) takes its turn behind the proofs already queued and runs on a free
// slot - it never shares a stream or workspace with a running proof.
static int prove_one(bn254s_ctx* c, int kind, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x,
                     const uint64_t* off, size_t n, bn254s_proof** out) {
  if (!c || !params || !scalars || !x || (kind != KIND_FQ && !off) || !out || n == 0 || params->struct_size != sizeof(bn254s_params))
    return BN254S_E_INVALID_ARG;
  *out = nullptr;
  return bn254s_prove_batch(c, kind, params, scalars, x, off, n, n, out);
}
int bn254s_prove_g1(bn254s_ctx* c, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x, const uint64_t* off,
                    size_t n, bn254s_proof** out) {
  return prove_one(c, KIND_G1, params, scalars, x, off, n, out);
}
// One process, several GPUs: proof i goes to context i mod n_ctx (proofs share no state), each context
// pipelines its share exactly like bn254s_prove_batch.  No inter-GPU traffic.
int bn254s_prove_batch_multi(bn254s_ctx** ctxs, size_t n_ctx, int kind, const bn254s_params* params, const uint64_t* scalars,
                             const uint64_t* x, const uint64_t* off, size_t n_total, size_t per_proof, bn254s_proof** proofs_out) {
  if (!ctxs || n_ctx == 0 || kind < 0 || kind > 2 || !params || !scalars || !x || (kind != KIND_FQ && !off) || !proofs_out ||
      n_total == 0 || per_proof == 0)
    return BN254S_E_INVALID_ARG;
  for (size_t g = 0; g < n_ctx; g++)
    if (!ctxs[g]) return BN254S_E_INVALID_ARG;
  const size_t n_proofs = (n_total + per_proof - 1) / per_proof;
  const size_t PW = stark_kind(kind).point_words;
  for (size_t i = 0; i < n_proofs; i++) proofs_out[i] = nullptr;
  std::vector<int> rcs(n_ctx, BN254S_OK);
  std::vector<std::thread> th;
  for (size_t g = 0; g < n_ctx; g++)
    th.emplace_back([&, g]() {
      // gather this context's share into contiguous job arrays (proof i of the share = global proof g + i * n_ctx)
      std::vector<u64> ls, lx, lo;
      std::vector<size_t> ids;
      for (size_t i = g; i < n_proofs; i += n_ctx) {
        const size_t b = i * per_proof, cnt = std::min(per_proof, n_total - b);
        if (cnt != per_proof && i + 1 != n_proofs) continue;  // (only the very last proof may be short)
        ids.push_back(i);
        ls.insert(ls.end(), scalars + 4 * b, scalars + 4 * (b + cnt));
        lx.insert(lx.end(), x + PW * b, x + PW * (b + cnt));
        if (off) lo.insert(lo.end(), off + PW * b, off + PW * (b + cnt));
      }
      if (ids.empty()) return;
      // a short last proof must stay last in its share: it is, since shares are in increasing global order
      std::vector<bn254s_proof*> out(ids.size(), nullptr);
      rcs[g] = bn254s_prove_batch(ctxs[g], kind, params, ls.data(), lx.data(), off ? lo.data() : nullptr, ls.size() / 4, per_proof,
                                  out.data());
      if (rcs[g] == BN254S_OK)
        for (size_t k = 0; k < ids.size(); k++) proofs_out[ids[k]] = out[k];
    });
  for (auto& t : th) t.join();
  int rc = BN254S_OK;
  for (size_t g = 0; g < n_ctx; g++)
    if (rcs[g] != BN254S_OK && rc == BN254S_OK) rc = rcs[g];
  if (rc != BN254S_OK)
    for (size_t i = 0; i < n_proofs; i++)
      if (proofs_out[i]) {
        delete proofs_out[i];
        proofs_out[i] = nullptr;
      }
  return rc;
}

int bn254s_prove_g2(bn254s_ctx* c, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x, const uint64_t* off,
                    size_t n, bn254s_proof** out) {
  return prove_one(c, KIND_G2, params, scalars, x, off, n, out);
}
int bn254s_prove_fq_exp(bn254s_ctx* c, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x, size_t n,
                        bn254s_proof** out) {
  return prove_one(c, KIND_FQ, params, scalars, x, nullptr, n, out);
}

int bn254s_proof_words(const bn254s_proof* p, const uint64_t** data, size_t* len) {
  if (!p || !data || !len) return BN254S_E_INVALID_ARG;
  *data = p->words.data();
  *len = p->words.size();
  return BN254S_OK;
}
int bn254s_proof_section(const bn254s_proof* p, int id, const uint64_t** data, size_t* len) {
  if (!p || !data || !len || id < 0 || id >= BN254S_SEC_COUNT) return BN254S_E_INVALID_ARG;
  *data = p->words.data() + p->sec_off[id];
  *len = p->sec_off[id + 1] - p->sec_off[id];
  return BN254S_OK;
}
int bn254s_proof_degree_bits(const bn254s_proof* p) { return p ? p->degree_bits : 0; }
int bn254s_proof_outputs(const bn254s_proof* p, const uint64_t** data, size_t* len) {
  if (!p || !data || !len) return BN254S_E_INVALID_ARG;
  *data = p->outputs.data();
  *len = p->outputs.size();
  return BN254S_OK;
}
int bn254s_proof_stage_ms(const bn254s_proof* p, const float** ms, size_t* n_stages) {
  if (!p || !ms || !n_stages) return BN254S_E_INVALID_ARG;
  *ms = p->stage_ms;
  *n_stages = ST_COUNT;
  return BN254S_OK;
}
const char* bn254s_stage_name(size_t stage) { return stage < ST_COUNT ? STAGE_NAMES[stage] : ""; }
size_t bn254s_proof_serialize(const bn254s_proof* p, uint8_t* buf, size_t cap) {
  if (!p) return 0;
  size_t need = p->words.size() * 8;
  if (buf && cap >= need) memcpy(buf, p->words.data(), need);  // hosts are little-endian
  return need;
}
void bn254s_proof_free(bn254s_proof* p) { delete p; }

int bn254s_generate_trace(bn254s_ctx* c, int kind, const uint64_t* scalars, const uint64_t* x, const uint64_t* off, size_t n,
                          uint32_t min_rows_log2, uint64_t* trace_out, uint64_t* outputs) {
  if (!c || kind < 0 || kind > 2 || !scalars || !x || (kind != KIND_FQ && !off) || n == 0 || !trace_out) return BN254S_E_INVALID_ARG;
  if (min_rows_log2 < 16) {  // the range-check table needs all 2^16 values (scalar_mul_stark.rs:71-87)
    c->set_err("min_rows_log2 must be >= 16");
    return BN254S_E_INVALID_ARG;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const StarkKind& sk = stark_kind(kind);
  const int PW = sk.point_words;
  const StarkShape& sh = sk.shape;
  size_t N = rows_for(n, min_rows_log2);
  const size_t in_words = n * (4 + 2 * (size_t)PW);
  u64* d_in = c->words("gt.in", in_words);
  u64* d_trace = c->words("gt.trace", (size_t)sh.W * N);
  u64* d_scr = c->words("gt.scratch", sk.trace_scratch_words(n));
  u64* d_out = c->words("gt.out", n * PW + 8);
  if (!d_in || !d_trace || !d_scr || !d_out) return BN254S_E_OOM;
  int* d_err = (int*)(d_out + n * PW);
  HIP_TRY(c, hipMemsetAsync(d_err, 0, 4, c->stream));
  std::string err;
  if (int rc = upload_and_generate(sk, scalars, x, off, n, d_in, d_trace, N, d_scr, d_out, d_err, c->stream, true, err)) {
    c->set_err(err);
    return rc;
  }
  int h_err = 0;
  HIP_TRY(c, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(trace_out, d_trace, (size_t)sh.W * N * 8, hipMemcpyDeviceToHost, c->stream));
  if (outputs) HIP_TRY(c, hipMemcpyAsync(outputs, d_out, n * (size_t)PW * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (h_err) {
    c->set_err("trace generation reported device error " + std::to_string(h_err));
    return h_err;
  }
  return BN254S_OK;
}
int bn254s_g1_generate_trace(bn254s_ctx* c, const uint64_t* scalars, const uint64_t* x, const uint64_t* off, size_t n,
                             uint32_t min_rows_log2, uint64_t* trace_out, uint64_t* outputs) {
  return bn254s_generate_trace(c, KIND_G1, scalars, x, off, n, min_rows_log2, trace_out, outputs);
}

}  // extern "C"

// loads this translation unit's code object (the HIP runtime defers that to the first launch otherwise)
void prover_module_warm() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_quotient_chunks));
}
