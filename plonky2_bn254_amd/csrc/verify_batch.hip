// bn254s_verify_batch: the native verifier for many proofs of one kind, parameter set and height (include/bn254_stark.h).
//
// Per proof the verifier has three parts (verify.hip): verify_front (shape, transcript, the AIR at zeta, proof of work: about
// 2 ms of host code), the query rounds (num_queries x ~220 Poseidon permutations plus the FRI arithmetic: ~50 ms on one host
// thread, and all of it independent per query) and verify_ctl (the claimed inputs / outputs against the CTL sums).  Here the
// fronts and the CTL checks of different proofs run on a few host threads and the query rounds of all proofs that passed their
// front run as two kernels over the functions of verify_query.h:
//   k_vb_merkle  one lane per (proof, query), the check (initial tree 0..2, FRI layer l) on blockIdx.y: one byte per check;
//   k_vb_fri     one lane per (proof, query): vq_fri_round, one code.
// The host merges bytes and codes into the per-query code (vq_merge_code) and takes the lowest failing query of each proof, so a
// proof gets the status and the text bn254s_verify_host gives it alone.  Without a context the query rounds run on the host
// threads as well.
//
// Device memory belongs to the call: allocated on entry, freed on every exit path (VbDevice), no named buffer of the context
// (that map is not safe against the workers of an open batch).  All work goes on the context's stream.
#include <atomic>
#include <chrono>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include "ctx.h"
#include "verify_query.h"

// Every lane of a block has the same `which`, hence the same number of permutations.  Lanes past the end work on the last item
// and drop the result: no lane leaves before the permutations are done.
__global__ __launch_bounds__(256) void k_vb_merkle(View v, const u64* __restrict__ words, size_t n_words,
                                                   const u64* __restrict__ recs, size_t rec_words, u32 n_items,
                                                   unsigned char* __restrict__ out) {
  const int which = (int)blockIdx.y;
  u32 item = blockIdx.x * 256u + threadIdx.x;
  const bool live = item < n_items;
  if (!live) item = n_items - 1;
  const u32 p = item / (u32)v.num_queries, q = item % (u32)v.num_queries;
  const bool ok = vq_merkle_check(v, words + (size_t)p * n_words, recs + (size_t)p * rec_words, q, which);
  if (live) out[(size_t)which * n_items + item] = ok ? 1 : 0;
}

__global__ __launch_bounds__(64) void k_vb_fri(View v, const u64* __restrict__ words, size_t n_words, const u64* __restrict__ recs,
                                               size_t rec_words, u32 n_items, int* __restrict__ out) {
  const u32 item = blockIdx.x * 64u + threadIdx.x;
  if (item >= n_items) return;
  const u32 p = item / (u32)v.num_queries, q = item % (u32)v.num_queries;
  out[item] = vq_fri_round(v, words + (size_t)p * n_words, recs + (size_t)p * rec_words, q);
}

static_assert(VQ_REC_QUERIES == BN254S_VERIFY_RECORD_HEAD, "the public header states the record layout");

namespace {

constexpr size_t VB_THREADS = 16;                      // host threads for the fronts and the CTL checks (not read from the machine)
constexpr size_t VB_CHUNK_BYTES = (size_t)256 << 20;   // proof words on the device at a time; a chunk never splits a proof

// f(i) for i < n on min(VB_THREADS, n) plain threads; f touches the state of proof i only
template <class F>
void vb_parallel(size_t n, F f) {
  const size_t nt = n < VB_THREADS ? n : VB_THREADS;
  if (nt <= 1) {
    for (size_t i = 0; i < n; i++) f(i);
    return;
  }
  std::atomic<size_t> next{0};
  auto run = [&]() {
    for (size_t i; (i = next.fetch_add(1)) < n;) f(i);
  };
  std::vector<std::thread> th;
  for (size_t t = 1; t < nt; t++) th.emplace_back(run);
  run();
  for (auto& t : th) t.join();
}

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct VbDevice {  // what a call holds on the device; released on every way out
  u64 *words = nullptr, *recs = nullptr;
  unsigned char* mk = nullptr;
  int* fri = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  ~VbDevice() {
    if (words) (void)hipFree(words);
    if (recs) (void)hipFree(recs);
    if (mk) (void)hipFree(mk);
    if (fri) (void)hipFree(fri);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

size_t chunk_by_size(size_t n_words) {
  const size_t k = VB_CHUNK_BYTES / 8 / n_words;
  return k ? k : 1;
}

// codes[k * num_queries + q] for the proofs words[idx[k]], records recs + idx[k] * rec_words.  ms: upload | k_vb_merkle | k_vb_fri.
int query_round_device(bn254s_ctx* c, const View& v, const u64* const* words, const u64* recs, const std::vector<size_t>& idx,
                       size_t chunk_proofs, int32_t* codes, float ms[3]) {
  const size_t n = idx.size(), nq = (size_t)v.num_queries, n_words = v.total, rec_words = vq_record_words((uint32_t)nq);
  const int checks = 3 + v.L;
  ms[0] = ms[1] = ms[2] = 0;
  if (n == 0) return BN254S_OK;
  size_t chunk = chunk_by_size(n_words);
  if (chunk_proofs && chunk_proofs < chunk) chunk = chunk_proofs;
  if (chunk > n) chunk = n;
  const size_t max_items = chunk * nq;
  if (max_items > ((size_t)1 << 30)) {
    c->set_err("verify_batch: too many queries in one chunk");
    return BN254S_E_UNSUPPORTED;
  }
  VbDevice d;
  if (hipMalloc(&d.words, chunk * n_words * 8) != hipSuccess || hipMalloc(&d.recs, chunk * rec_words * 8) != hipSuccess ||
      hipMalloc(&d.mk, (size_t)checks * max_items) != hipSuccess || hipMalloc(&d.fri, max_items * sizeof(int)) != hipSuccess) {
    (void)hipGetLastError();
    c->set_err("verify_batch: hipMalloc failed");
    return BN254S_E_OOM;
  }
  for (hipEvent_t& e : d.ev) HIP_TRY(c, hipEventCreate(&e));
  std::vector<unsigned char> h_mk((size_t)checks * max_items);
  std::vector<int> h_fri(max_items);
  hipStream_t st = c->stream;
  for (size_t p0 = 0; p0 < n; p0 += chunk) {
    const size_t np = n - p0 < chunk ? n - p0 : chunk;
    const u32 n_items = (u32)(np * nq);
    HIP_TRY(c, hipEventRecord(d.ev[0], st));
    for (size_t k = 0; k < np; k++) {
      HIP_TRY(c, hipMemcpyAsync(d.words + k * n_words, words[idx[p0 + k]], n_words * 8, hipMemcpyHostToDevice, st));
      HIP_TRY(c, hipMemcpyAsync(d.recs + k * rec_words, recs + idx[p0 + k] * rec_words, rec_words * 8, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(c, hipEventRecord(d.ev[1], st));
    k_vb_merkle<<<dim3((n_items + 255) / 256, (unsigned)checks), 256, 0, st>>>(v, d.words, n_words, d.recs, rec_words, n_items, d.mk);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(d.ev[2], st));
    k_vb_fri<<<(n_items + 63) / 64, 64, 0, st>>>(v, d.words, n_words, d.recs, rec_words, n_items, d.fri);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(d.ev[3], st));
    HIP_TRY(c, hipMemcpyAsync(h_mk.data(), d.mk, (size_t)checks * n_items, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(h_fri.data(), d.fri, (size_t)n_items * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    for (int s = 0; s < 3; s++) {
      float t = 0;
      HIP_TRY(c, hipEventElapsedTime(&t, d.ev[s], d.ev[s + 1]));
      ms[s] += t;
    }
    for (u32 item = 0; item < n_items; item++)
      codes[p0 * nq + item] =
          vq_merge_code(v.L, [&](int which) { return h_mk[(size_t)which * n_items + item] != 0; }, h_fri[item]);
  }
  return BN254S_OK;
}

void put_err(char* err, size_t stride, size_t i, const std::string& text) {
  if (!err) return;
  strncpy(err + i * stride, text.c_str(), stride - 1);
  err[i * stride + stride - 1] = 0;
}

bool params_ok(int kind, const bn254s_params* params, uint32_t degree_bits) {
  return kind >= 0 && kind <= 2 && params && params->struct_size == sizeof(bn254s_params) && degree_bits >= 7 && degree_bits <= 30;
}

}  // namespace

extern "C" {

int bn254s_verify_batch(bn254s_ctx* c, int kind, const bn254s_params* params, uint32_t degree_bits, const uint64_t* const* words,
                        size_t n_words, const uint64_t* scalars, const uint64_t* x, const uint64_t* offset, const uint64_t* outputs,
                        const size_t* n_jobs, size_t n_proofs, int32_t* status, char* err, size_t err_stride) {
  if (!params_ok(kind, params, degree_bits) || !words || !scalars || !x || (kind != KIND_FQ && !offset) || !outputs || !n_jobs ||
      n_proofs == 0 || !status || (err && err_stride == 0))
    return BN254S_E_INVALID_ARG;
  for (size_t i = 0; i < n_proofs; i++)
    if (!words[i] || n_jobs[i] == 0) return BN254S_E_INVALID_ARG;
  if (params->num_challenges != 2 || params->rate_bits != 1) {
    if (c) c->set_err("only num_challenges = 2, rate_bits = 1 are supported");
    return BN254S_E_UNSUPPORTED;
  }
  if (c && hipSetDevice(c->device) != hipSuccess) return BN254S_E_HIP;
  const bn254s_params& P = *params;
  const size_t PW = (size_t)stark_kind(kind).point_words, nq = P.num_queries, rec_words = vq_record_words(P.num_queries);
  struct PerProof {
    int rc = BN254S_OK;
    std::string text;
    View v;
    u64 ctl_ch[4];
    size_t job0 = 0;
  };
  std::vector<PerProof> pp(n_proofs);
  for (size_t i = 1; i < n_proofs; i++) pp[i].job0 = pp[i - 1].job0 + n_jobs[i - 1];
  std::vector<u64> recs(n_proofs * rec_words);
  auto front = [&](size_t i) {
    pp[i].rc = verify_front(nullptr, kind, P, (int)degree_bits, words[i], n_words, pp[i].v, &recs[i * rec_words], pp[i].ctl_ch,
                            pp[i].text);
  };
  auto ctl = [&](size_t i) {
    if (pp[i].rc != BN254S_OK) return;
    const size_t j = pp[i].job0;
    pp[i].rc = verify_ctl(kind, pp[i].v, words[i], pp[i].ctl_ch, scalars + 4 * j, x + PW * j, offset ? offset + PW * j : nullptr,
                          outputs + PW * j, n_jobs[i], pp[i].text);
  };
  auto reject = [&](size_t i, int L, const int32_t* codes) {  // the lowest failing query decides, as the loop over q does
    for (size_t q = 0; q < nq; q++)
      if (codes[q]) {
        pp[i].rc = BN254S_E_VERIFY;
        pp[i].text = vq_code_text(L, codes[q]);
        return;
      }
  };
  float ms[5] = {0, 0, 0, 0, 0};  // front | upload | k_vb_merkle | k_vb_fri | CTL
  int call_rc = BN254S_OK;
  if (!c) {  // no GPU: front, query rounds and CTL of a proof on one host thread
    vb_parallel(n_proofs, [&](size_t i) {
      front(i);
      if (pp[i].rc != BN254S_OK) return;
      std::vector<int32_t> codes(nq);
      for (uint32_t q = 0; q < nq; q++) codes[q] = verify_query_host(pp[i].v, words[i], &recs[i * rec_words], q);
      reject(i, pp[i].v.L, codes.data());
      ctl(i);
    });
  } else {
    double t0 = now_ms();
    vb_parallel(n_proofs, front);
    ms[0] = (float)(now_ms() - t0);
    std::vector<size_t> idx;  // a proof that failed its front is not sent to the device
    for (size_t i = 0; i < n_proofs; i++)
      if (pp[i].rc == BN254S_OK) idx.push_back(i);
    if (!idx.empty()) {
      std::vector<int32_t> codes(idx.size() * nq);
      call_rc = query_round_device(c, pp[idx[0]].v, words, recs.data(), idx, 0, codes.data(), ms + 1);
      if (call_rc == BN254S_OK)
        for (size_t k = 0; k < idx.size(); k++) reject(idx[k], pp[idx[k]].v.L, &codes[k * nq]);
    }
    if (call_rc == BN254S_OK) {
      t0 = now_ms();
      vb_parallel(n_proofs, ctl);
      ms[4] = (float)(now_ms() - t0);
      std::lock_guard<std::mutex> lk(c->err_mu);
      memcpy(c->vb_ms, ms, sizeof(ms));
    }
  }
  if (call_rc != BN254S_OK) {  // the call itself failed (the context holds the reason): no verdicts
    for (size_t i = 0; i < n_proofs; i++) {
      status[i] = call_rc;
      put_err(err, err_stride, i, "");
    }
    return call_rc;
  }
  int ret = BN254S_OK;
  bool named = false;
  for (size_t i = 0; i < n_proofs; i++) {
    status[i] = pp[i].rc;
    put_err(err, err_stride, i, pp[i].rc == BN254S_OK ? std::string() : pp[i].text);
    if (pp[i].rc == BN254S_OK) continue;
    if (pp[i].rc != BN254S_E_VERIFY && (ret == BN254S_OK || ret == BN254S_E_VERIFY)) ret = pp[i].rc;  // e.g. an internal AIR error
    if (ret == BN254S_OK) ret = BN254S_E_VERIFY;
    if (!named && c) {
      c->set_err("proof " + std::to_string(i) + ": " + pp[i].text);
      named = true;
    }
  }
  return ret;
}

// ---- debug entry points (in the style of fri_selftest.hip; used by the tests) --------------------------------------------------
int bn254s_selftest_verify_front(int kind, const bn254s_params* params, uint32_t degree_bits, const uint64_t* words, size_t n_words,
                                 uint64_t* record_out, size_t record_cap) {
  if (!params_ok(kind, params, degree_bits) || !words || !record_out || record_cap < vq_record_words(params->num_queries))
    return BN254S_E_INVALID_ARG;
  if (params->num_challenges != 2 || params->rate_bits != 1) return BN254S_E_UNSUPPORTED;
  View v;
  u64 ctl_ch[4];
  std::string text;
  return verify_front(nullptr, kind, *params, (int)degree_bits, words, n_words, v, record_out, ctl_ch, text);
}

int bn254s_selftest_query_round(bn254s_ctx* c, int kind, const bn254s_params* params, uint32_t degree_bits,
                                const uint64_t* const* words, size_t n_words, const uint64_t* records, size_t n_proofs,
                                size_t chunk_proofs, int32_t* codes_out) {
  if (!params_ok(kind, params, degree_bits) || !words || !records || !codes_out || n_proofs == 0) return BN254S_E_INVALID_ARG;
  if (params->num_challenges != 2 || params->rate_bits != 1) return BN254S_E_UNSUPPORTED;
  View v;
  if (!make_view(kind, *params, (int)degree_bits, v) || v.total != n_words) return BN254S_E_INVALID_ARG;
  const size_t nq = params->num_queries, rec_words = vq_record_words(params->num_queries);
  for (size_t i = 0; i < n_proofs; i++) {
    if (!words[i]) return BN254S_E_INVALID_ARG;
    const u64* rec = records + i * rec_words;
    for (size_t k = 0; k < rec_words; k++)  // field words below p; a query index is what addresses the caps: below 2^log_m2
      if (rec[k] >= GL_P || (k >= (size_t)VQ_REC_QUERIES && (rec[k] >> v.log_m2))) return BN254S_E_INVALID_ARG;
  }
  if (!c) {
    vb_parallel(n_proofs, [&](size_t i) {
      for (uint32_t q = 0; q < nq; q++) codes_out[i * nq + q] = verify_query_host(v, words[i], records + i * rec_words, q);
    });
    return BN254S_OK;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  std::vector<size_t> idx(n_proofs);
  for (size_t i = 0; i < n_proofs; i++) idx[i] = i;
  float ms[3];
  return query_round_device(c, v, words, records, idx, chunk_proofs, codes_out, ms);
}

const char* bn254s_selftest_query_text(int n_layers, int code) {
  if (n_layers < 0 || n_layers > FRI_MAX_LAYERS || code < 0 || code > 4 + 2 * n_layers) return nullptr;
  return code ? vq_code_text(n_layers, code) : "";
}

int bn254s_selftest_verify_batch_ms(bn254s_ctx* c, float* ms_out) {
  if (!c || !ms_out) return BN254S_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->err_mu);
  memcpy(ms_out, c->vb_ms, sizeof(c->vb_ms));
  return BN254S_OK;
}

}  // extern "C"
