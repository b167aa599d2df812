// eg_hip.hip -- host side of libeg_hip.so: context, the plan-driven verification engine and the C ABI
// declared in include/eg_hip.h.  One process drives one GPU (one rank per GPU under torch.distributed);
// everything is launched on a single HIP stream, per chunk of ballots:
//   decode -> canonical checks -> derived points -> [ group equations -> transcript hashing ] x stages
//   -> status -> tally
// There is no CPU fallback: every numeric result comes out of the kernels in kernels.cuh.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <condition_variable>
#include <deque>
#include <list>
#include <unordered_map>
#include <vector>

#include "../../include/eg_hip.h"
#include "host_plan.hpp"
#include "wire_json.hpp"
#include "kernels.cuh"
#include "latency_kernels.cuh"
#include "pippenger.cuh"
#include "dlog_kernels.cuh"
#include "group_tally_kernels.cuh"
#include "share_combine_kernels.cuh"
#include "weed_kernels.cuh"
#include "weed_index_kernels.cuh"
#include "ed25519_kernels.cuh"
#include "roll_kernels.cuh"
#include "merkle_kernels.cuh"
#include "merkle_audit_kernels.cuh"
#include "merkle_grow_kernels.cuh"
#include "open_kernels.cuh"
#include "shuffle_kernels.cuh"

using namespace eg;

// defined in eg_gen.hip (separate translation unit so the two compile in parallel)
void eg_launch_qv_encrypt(int blocks, hipStream_t s, u64 seed0, size_t n, int n_options, u64 credits, const u32* votes, u64 rng_skip,
                          int vote_rings, int vote_main, int vote_ring, const u32* d_vote_desc, int credit_rings, int credit_main,
                          int credit_ring, const u32* d_credit_desc, int pre_sumsq, const uint4* tabG, const uint4* tabK,
                          const u32* prefixes, u32* out, u32 stride_words, u32 vote_words, u32 credit_words, u32* gws);
void eg_launch_choice_encrypt(int blocks, hipStream_t s, u64 seed0, size_t n, int n_options, int single, int n_selected,
                              const u32* selection, u64 rng_skip, const uint4* tabG, const uint4* tabK, const u32* prefixes, int pre_main, int pre_ring,
                              int pre_logeq, u32* out, u32 stride_words, u32* gws);
void eg_launch_commit_equiv_prove(int blocks, hipStream_t s, u64 seed0, size_t n, u64 rng_skip, const u64* values, const uint4* tabG,
                                  const uint4* tabK, const uint4* tabH, const u32* prefixes, int pre, u32* out, u32* blindings);
void eg_launch_zero_prove(int blocks, hipStream_t s, u64 seed0, size_t n, u64 rng_skip, const uint4* tabG, const uint4* tabK,
                          const u32* prefixes, int pre, u32* out);
void eg_launch_range_prove(int blocks, hipStream_t s, u64 seed0, size_t n, u64 rng_skip, const u64* values, int n_rings, int pre_main,
                           int pre_ring, const u32* d_desc, const uint4* tabG, const uint4* tabK, const u32* prefixes, u32* out,
                           u32 stride_words, u32* gws);
void eg_launch_sumsq_prove(int blocks, hipStream_t s, u64 seed0, size_t n, u64 rng_skip, int n_values, const u64* values, int pre,
                           const uint4* tabG, const uint4* tabK, const u32* prefixes, u32* out, u32 stride_words, u32* gws);
void eg_launch_share_prove(int blocks, hipStream_t s, u64 seed0, size_t n, u64 rng_skip, const u32 secret[8], const u32 participant_key[8],
                           const u32* ct_random, const uint4* tabG, const u32* prefixes, int pre, u32* out, unsigned char* ok, u32* gws);
void eg_launch_choice_open(int blocks, hipStream_t s, u64 seed0, size_t n, int n_options, int single, int n_selected, const u32* selection,
                           u64 rng_skip, unsigned long long* values, u32* rand);
void eg_launch_qv_open(int blocks, hipStream_t s, u64 seed0, size_t n, int n_options, u64 credits, const u32* votes, u64 rng_skip,
                       u64 draws_per_vote, unsigned long long* values, u32* rand);
unsigned eg_gen_choice_ws_words(int n_options);
unsigned eg_gen_qv_ws_words(int n_options, unsigned max_rings, unsigned max_responses);

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIPCHK(x)                                                                                   \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess)                                                                           \
      return fail(EG_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_) + " (" + __FILE__ + ":" + std::to_string(__LINE__) + ")"); \
  } while (0)

#define TRY_(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)
// An entry point that works on SEVERAL devices (the multi-GPU calls, a JSON stream with one lane per GPU) leaves the calling thread's current
// device as it found it: a host that drives its own HIP work (or torch) on that thread must not find another device selected afterwards.
struct KeepDevice {
  int dev = -1;
  KeepDevice() { if (hipGetDevice(&dev) != hipSuccess) { dev = -1; (void)hipGetLastError(); } }
  ~KeepDevice() { if (dev >= 0) (void)hipSetDevice(dev); }
};
// runs at scope exit, on every path (early returns of HIPCHK included)
struct ScopeExit {
  std::function<void()> fn;
  ~ScopeExit() { if (fn) fn(); }
};
// Every run-time knob of the library, read from the environment in ONE place and at two moments only: eg_init (the context keeps a copy)
// and the creation of a params object (the engine keeps its own copy, so a host may change the environment between two elections).  No
// entry point reads the environment per call.  The table in include/eg_hip.h ("Run-time knobs") is the documentation; keep it in step.
struct Knobs {
  int teeth = 0;                    // EG_TEETH            0 = by plan (5 or 6)
  int streams = 2;                  // EG_STREAMS          work sets (1 or 2)
  size_t chunk = 0;                 // EG_CHUNK            0 = by plan and memory
  int ring_group = -1;              // EG_RING_GROUP       -1 = by plan (off below 256 options), 0 = off, g = rings per group
  int comb_big_bits = -1;           // EG_COMB_BIG_BITS    -1 = EG_COMB_BITS_BIG
  long long comb_big_min = -1;      // EG_COMB_BIG_MIN     -1 = 2^19 items
  int msm_blocks_per_cu = 32;       // EG_MSM_BLOCKS_PER_CU
  size_t msm_lanes = (size_t)1 << 17;       // EG_MSM_LANES
  size_t msm_bucket_min = (size_t)1 << 20;  // EG_MSM_BUCKET_MIN
  size_t json_ring_kb = 0, json_window_kb = 0;   // EG_JSON_RING_KB, EG_JSON_WINDOW_KB   0 = 1 GiB ring, 96 MiB windows
  size_t json_growth = 150;         // EG_JSON_GROWTH      per cent
  size_t json_first_min = 0;        // EG_JSON_FIRST_MIN   0 = the stream's default (stream_begin)
  size_t json_odd_max_mb = 256;     // EG_JSON_ODD_MAX_MB  text of wrong-shape ballots a JSON stream keeps for the object path
  bool json_trace = false;          // EG_JSON_TRACE
  bool allow_any_arch = false;      // EG_ALLOW_ANY_ARCH
};
static Knobs read_knobs() {
  Knobs k;
  auto num = [](const char* name, long long dflt) { const char* v = getenv(name); return v && *v ? strtoll(v, nullptr, 10) : dflt; };
  { const long long t = num("EG_TEETH", 0); if (t == 5 || t == 6) k.teeth = (int)t;
#ifdef EG_TEETH7
    if (t == 7) k.teeth = 7;
#endif
  }
  if (getenv("EG_STREAMS")) k.streams = num("EG_STREAMS", 2) >= 2 ? 2 : 1;
  k.chunk = (size_t)std::max<long long>(0, num("EG_CHUNK", 0));
  if (getenv("EG_RING_GROUP")) k.ring_group = (int)std::max<long long>(0, num("EG_RING_GROUP", 0));
  if (getenv("EG_COMB_BIG_BITS")) k.comb_big_bits = (int)num("EG_COMB_BIG_BITS", -1);
  if (getenv("EG_COMB_BIG_MIN")) k.comb_big_min = std::max<long long>(0, num("EG_COMB_BIG_MIN", -1));
  k.msm_blocks_per_cu = (int)std::max<long long>(1, num("EG_MSM_BLOCKS_PER_CU", 32));
  k.msm_lanes = (size_t)std::max<long long>(1, num("EG_MSM_LANES", 1 << 17));
  k.msm_bucket_min = (size_t)std::max<long long>(0, num("EG_MSM_BUCKET_MIN", 1 << 20));
  k.json_ring_kb = (size_t)std::max<long long>(0, num("EG_JSON_RING_KB", 0));
  k.json_window_kb = (size_t)std::max<long long>(0, num("EG_JSON_WINDOW_KB", 0));
  k.json_growth = (size_t)std::max<long long>(0, num("EG_JSON_GROWTH", 150));
  k.json_first_min = (size_t)std::max<long long>(0, num("EG_JSON_FIRST_MIN", 0));
  k.json_odd_max_mb = (size_t)std::max<long long>(1, num("EG_JSON_ODD_MAX_MB", 256));
  k.json_trace = getenv("EG_JSON_TRACE") != nullptr;
  k.allow_any_arch = getenv("EG_ALLOW_ANY_ARCH") != nullptr;
  return k;
}
// Fault points: places where a TEST build can make a call fail on purpose.  The shipped library has none - the macro is the constant
// false - and holds no name of a switch; tests/faultlib builds a second library with -DEG_FAULT_POINTS_H=<its header>, which defines the macro.
#ifdef EG_FAULT_POINTS_H
#include EG_FAULT_POINTS_H
#else
#define EG_FAULT_POINT(name) false
#endif
enum { PROF_CALL = 0, PROF_MSM = 1, PROF_TABLES = 2 };
struct ProfSpan { hipEvent_t a, b; int kind; };

struct eg_ctx {
  std::recursive_mutex mu;   // serialises the C entry points of one context (and of the params created on it)
  Knobs knobs;               // the environment as eg_init found it (read_knobs)
  std::atomic<int> refs{1};  // the caller's reference + one per live params object
  int device = 0;
  hipStream_t stream = nullptr;
  int cus = 0;
  std::string name;
  uint4* tabG = nullptr;     // fixed-base comb table of the generator, EG_COMB_BITS wide (points at the first entry; comb_table_build)
  uint4* tabG_big = nullptr; // the same, big_bits wide: built when the first large batch arrives (ensure_big_tables)
  int big_bits = EG_COMB_BITS_BIG;      // 0: never build wide tables (EG_COMB_BIG_BITS)
  size_t big_min = (size_t)1 << 19;     // an engine that has verified this many items gets the wide tables (EG_COMB_BIG_MIN)
  bool big_failed = false;              // the wide tables did not fit the device memory: do not try again
  u32* gen_words = nullptr;  // generator as PT_WORDS limbs
  int resident_blocks = 0;   // blocks of the equation kernel that the chip holds at once (two per CU)
  int msm_blocks = 0;        // grid of the table / equation kernels: EG_GRID_OVERSUBSCRIBE x resident_blocks, each block striding over its share
  uint4* ws = nullptr;       // per-lane workspace of those kernels (msm_blocks * WS_QUADS * NT uint4)
  // The workspace is shared by EVERY engine of the context and by the primitive tier, in two halves (work set k of an engine uses half k;
  // a one-set call and k_prim_msm use both).  Calls are serialised on the host by `mu`, but their kernels are not: a JSON stream's
  // submissions, `_device` calls on caller streams and the work sets' own streams all run asynchronously.  Every user therefore makes its
  // stream wait for the last user of the halves it is about to write (ws_acquire) and leaves an event behind (ws_release): the GPU side
  // is ordered without any host synchronisation, whatever stream, engine or thread the previous user was.
  hipEvent_t ws_done[2] = {nullptr, nullptr};
  hipStream_t ws_last[2] = {nullptr, nullptr};
  bool ws_used[2] = {false, false};
  void* prim_scratch = nullptr;   // device scratch of the primitive tier, kept between calls and grown on demand (prim_bufs)
  size_t prim_scratch_bytes = 0;
  bool prof = false;
  bool prof_serial = false;    // eg_profile_enable(ctx, 2): chunks one after the other on one work set, so that a launch's duration is its own
  std::vector<ProfSpan> spans;
  std::vector<hipEvent_t> event_pool;
  double msm_ms = 0, all_ms = 0, tables_ms = 0;
  uint64_t msm_launches = 0, tables_launches = 0;
};

// see eg_ctx::ws_done.  halves: bit k = half k of the workspace.  Called under the context's lock.
static int ws_acquire(eg_ctx* c, unsigned halves, hipStream_t s) {
  for (int h = 0; h < 2; ++h)
    if (((halves >> h) & 1u) && c->ws_used[h] && c->ws_last[h] != s) HIPCHK(hipStreamWaitEvent(s, c->ws_done[h], 0));
  return EG_OK;
}
static int ws_release(eg_ctx* c, unsigned halves, hipStream_t s) {
  for (int h = 0; h < 2; ++h)
    if ((halves >> h) & 1u) { HIPCHK(hipEventRecord(c->ws_done[h], s)); c->ws_used[h] = true; c->ws_last[h] = s; }
  return EG_OK;
}

static int prof_begin(eg_ctx* c, hipStream_t s, int kind, size_t* idx) {
  if (!c->prof) return EG_OK;
  hipEvent_t a, b;
  for (hipEvent_t* e : {&a, &b}) {
    if (!c->event_pool.empty()) { *e = c->event_pool.back(); c->event_pool.pop_back(); }
    else HIPCHK(hipEventCreate(e));
  }
  HIPCHK(hipEventRecord(a, s));
  *idx = c->spans.size();
  c->spans.push_back({a, b, kind});
  return EG_OK;
}
static int prof_end(eg_ctx* c, hipStream_t s, size_t idx) {
  if (!c->prof) return EG_OK;
  HIPCHK(hipEventRecord(c->spans[idx].b, s));
  return EG_OK;
}

template <class T>
static int upload(T** dptr, const std::vector<T>& v, hipStream_t s) {
  *dptr = nullptr;
  const size_t bytes = std::max<size_t>(v.size(), 1) * sizeof(T);
  HIPCHK(hipMalloc((void**)dptr, bytes));
  if (!v.empty()) HIPCHK(hipMemcpyAsync(*dptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
  return EG_OK;
}

// Builds the comb table of one fixed base (kernels.cuh: k_comb_window_bases + k_build_fixed_table) on stream s and waits for it
// (the scratch of the batched inversion is released before returning).  *out points at the first entry; the allocation starts
// COMB_HEADER_QUADS uint4 earlier (a whole cache line, so that the 128-byte entries stay line-aligned; the table's header is the
// last uint4 of it): release with comb_table_free.
static void comb_table_free(uint4* tab) { if (tab) (void)hipFree(tab - COMB_HEADER_QUADS); }
static int comb_table_build(const u32* d_base_words, int bits, hipStream_t s, uint4** out, bool soft_nomem = false) {
  *out = nullptr;
  if (bits < 8 || bits > 26) return fail(EG_ERR_BAD_ARG, "comb width out of range");
  const int windows = comb_windows(bits), entries = comb_entries(bits);
  const size_t lanes = (size_t)windows * (entries / COMB_RUN);
  uint4* base = nullptr;
  u32 *d_bases = nullptr, *scratch = nullptr;
  hipError_t he = hipMalloc((void**)&base, ((size_t)windows * entries * 8 + COMB_HEADER_QUADS) * sizeof(uint4));
  if (he == hipSuccess) he = hipMalloc((void**)&d_bases, (size_t)windows * PT_WORDS * sizeof(u32));
  if (he == hipSuccess) he = hipMalloc((void**)&scratch, (size_t)COMB_RUN * EG_NL * lanes * sizeof(u32));
  if (he != hipSuccess) {
    if (base) (void)hipFree(base);
    if (d_bases) (void)hipFree(d_bases);
    if (scratch) (void)hipFree(scratch);
    if (he == hipErrorOutOfMemory && soft_nomem) { (void)hipGetLastError(); return EG_ERR_NOMEM; }
    HIPCHK(he);
  }
  hipLaunchKernelGGL(k_comb_window_bases, dim3(1), dim3(64), 0, s, d_base_words, bits, d_bases);
  hipLaunchKernelGGL(k_build_fixed_table, dim3((unsigned)((lanes + NT - 1) / NT)), dim3(NT), 0, s, d_bases, bits, base + COMB_HEADER_QUADS, scratch);
  const hipError_t se = hipStreamSynchronize(s);
  (void)hipFree(d_bases); (void)hipFree(scratch);
  if (se != hipSuccess) { (void)hipFree(base); HIPCHK(se); }
  *out = base + COMB_HEADER_QUADS;
  return EG_OK;
}

// ---------------------------------------------------------------------------------------------------------------
using eghost::StageDev; using eghost::LevelDev;
using eghost::FAM_TABLE1; using eghost::FAM_TABLEN; using eghost::FAM_DIRECT1; using eghost::FAM_GENERIC; using eghost::FAM_ENCODE; using eghost::N_FAM;
using eghost::EG_MULTI_GROUP; using eghost::job_family;

struct Engine {
  eg_ctx* ctx = nullptr;
  eghost::Plan plan;
  int n_options = 0;
  // device plan
  egplan::WireItem *d_pt_items = nullptr, *d_sc_items = nullptr;
  egplan::DeriveClass* d_dclasses = nullptr;
  egplan::DeriveTerm* d_dterms = nullptr;
  egplan::JobClass* d_jobs = nullptr;
  egplan::VarTerm* d_vterms = nullptr;
  egplan::HashInst* d_insts = nullptr;
  egplan::HashOp* d_ops = nullptr;
  egplan::StatusRule* d_rules = nullptr;
  u32* d_tally_slots = nullptr;
  u32* d_tally_items = nullptr;                // wire item behind every tally slot (group_tally_host.hpp: tally_items): what the per-group tally reads
  bool weed_keys_ok = false;                   // the B item of every tally ciphertext is its R item + 1 (weed_host.hpp: key_items), checked at creation
  unsigned short* d_base_slots = nullptr;      // FlatPlan::build_slots: point slots by the stage that builds their tables
  egplan::SumBase* d_sum_bases = nullptr;      // FlatPlan::sums / sum_members (members as table slots)
  unsigned short* d_sum_members = nullptr;
  egplan::SumBase* d_acc_sums = nullptr;       // ring-group walk: FlatPlan::acc_sums / acc_members
  unsigned short* d_acc_members = nullptr;
  int n_sums = 0;
  unsigned short* d_defer_slots = nullptr;
  int max_defer = 0;
  unsigned char* d_blob = nullptr;
  uint4 *d_tabK = nullptr, *d_cpts = nullptr;   // d_tabK: comb table of the election key (first entry; see comb_table_build)
  uint4* d_tabK_big = nullptr;                 // its wide form, built with the context's (ensure_big_tables)
  uint4 *d_tabH = nullptr, *d_tabH_big = nullptr;   // plans with a third fixed base H (Plan::h_srcs): its comb tables, as K's; else null
  egplan::ScalarSrc* d_h_srcs = nullptr;       // Plan::h_srcs
  u32* d_h_words = nullptr;                    // [PT_WORDS..2 PT_WORDS) H (k_setup_points writes the generator in front)
  bool use_big = false;                        // this call reads the wide tables (one launch, one width: all of G, K and H, or none)
  size_t items_seen = 0;                       // items verified by this engine so far (the wide tables are built once it passes ctx->big_min)
  u32* d_prefixes = nullptr;
  u32* d_key_words = nullptr;   // [0..PT_WORDS) generator, [PT_WORDS..2 PT_WORDS) key
  std::vector<StageDev> stages;
  std::vector<LevelDev> levels;
  int prefix_inst_first = 0, prefix_inst_count = 0;
  // Chunk workspace: TWO sets, each with its own stream.  Consecutive chunks of a call alternate between the sets, so that the launch
  // tail of one chunk's kernels (the last blocks of a grid leave most CUs idle) is filled by the other chunk's kernels; the sets join
  // the caller's stream at the end of the call (fork / join with events).  Set 1 tallies into its own accumulator, which the join
  // adds to the running tally: the order of the additions is fixed by the code, not by timing.  (EG_STREAMS=1: one set, one stream.)
  struct WorkSet {
    uint4 *pts = nullptr, *cmp = nullptr, *chal = nullptr;
    u32 *states = nullptr, *flags = nullptr, *bad_item = nullptr;
    uint4 *btab = nullptr, *dpt = nullptr, *sacc = nullptr;
    u32* encw = nullptr;
    u32* partial = nullptr;
    u32* tally = nullptr;      // set 0: the engine's running tally; set 1: this call's share, added to set 0's at the join
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
  } set[2];
  int n_sets = 2;
  bool fused_tail = false;    // the stages end with k_encode_hash (engine_create)
  Knobs knobs;                 // the environment as the creation of this params object found it (read_knobs)
  uint8_t key_bytes[32] = {0}; // the election key as given (canonical encoding): two params objects belong to one election if these agree
  int teeth = 6;               // comb shape of the per-ballot tables (plan_teeth: 5 x 51 when a table serves two products, else 6 x 43)
  hipEvent_t fork = nullptr;
  u32 cap = 0, max_cap = 0;
  int tally_blocks = 64;
  u32* tally = nullptr;        // [2n][PT_WORDS] running tally (extended points) = set[0].tally
  u32* tally_saved = nullptr;  // [2n][PT_WORDS] the running tally set aside while a host call computes its per-batch tally
  u32* tally_saved2 = nullptr; // the same for the JSON entry points, which call the host form piece by piece
  u32* tally_saved3 = nullptr; // the running tally as a multi-GPU call found it (TallyRollback: put back if any slab fails)
  u32* d_tally_enc = nullptr;  // [2n][8] device staging of engine_tally_encode (no allocation per call)
  uint8_t* json_ring = nullptr;        // pinned staging of the JSON entry points: a ring of packed ballots that the parser threads fill
  size_t json_ring_bytes = 0;          // window by window while earlier windows are uploaded and verified
  u32* json_status_ring = nullptr;     // pinned verdicts of the ballots in the ring
  size_t json_ring_ballots = 0;
  hipStream_t json_ctl[2] = {nullptr, nullptr};   // control streams of consecutive windows (fork / join of a window's chunks)
  struct eg_json_stream* stream_open = nullptr;   // the JSON stream (eg_verify_json_begin ... _end) that owns this engine's work sets, ring and tally just now
  // LONG calls - the ones that do not hold the context's lock from start to end: a one-shot JSON call (its worker thread takes the lock piece
  // by piece) and a multi-GPU call (one host thread per slab) - hold this mutex for their whole length; every other entry point on the
  // params object WAITS for them (EG_WAIT_LONG).  `reserved` marks the engine as held by a multi-GPU call (set and cleared under the
  // context's lock): between the moment such a call sets the running tallies aside and its merge or roll-back, nobody else may verify, tally
  // or open a stream on the object.
  std::mutex long_call_mu;
  bool reserved = false;
  // the tail of the last asynchronous call that touched the running tally (engine_touch): what a later call on ANOTHER stream has to wait
  // for instead of draining the whole device (TallyRollback)
  hipEvent_t last_done = nullptr, saved_ev = nullptr;
  bool last_used = false;
  // staging for the host-pointer API
  hipStream_t copy_stream = nullptr;
  unsigned char* d_wire = nullptr;
  u32* d_status = nullptr;
  size_t staging_ballots = 0;
  // generators: per-lane workspace (grown on demand) and the ring shapes of the two range proofs of a QV ballot
  u32* gen_ws = nullptr;
  size_t gen_ws_bytes = 0;
  u32* d_gen_desc = nullptr;
  // small-batch path (k_ballot_small): the stage and level tables on the device, the block size the plan asks for, and the workspace of
  // the equations without a comb table (grown on demand; null for plans that have none)
  StageDev* d_small_stages = nullptr;
  LevelDev* d_small_levels = nullptr;
  int small_threads = 0;
  bool small_needs_ws = false;
  uint4* small_ws = nullptr;
  size_t small_ws_ballots = 0;
};

static int grid_for(size_t lanes, int cap_blocks);
// blocks of a generator launch and its per-lane workspace: at most ~2 GiB of scratch, whatever the election's size
static int gen_workspace(Engine* e, size_t n, unsigned words, int* blocks_out) {
  const size_t budget = (size_t)2 << 30;
  int blocks = grid_for(n, e->ctx->cus * 4);
  const size_t per_block = (size_t)NT * words * sizeof(u32);
  if ((size_t)blocks * per_block > budget) blocks = (int)std::max<size_t>(1, budget / per_block);
  const size_t need = (size_t)blocks * per_block;
  if (need > e->gen_ws_bytes) {
    HIPCHK(hipDeviceSynchronize());     // an earlier generator launch may still use the old slice
    if (e->gen_ws) (void)hipFree(e->gen_ws);
    e->gen_ws = nullptr; e->gen_ws_bytes = 0;
    HIPCHK(hipMalloc((void**)&e->gen_ws, need));
    e->gen_ws_bytes = need;
  }
  *blocks_out = blocks;
  return EG_OK;
}

static void engine_free(Engine* e) {
  if (!e) return;
  void* ptrs[] = {e->d_pt_items, e->d_sc_items, e->d_dclasses, e->d_dterms, e->d_jobs, e->d_vterms, e->d_insts, e->d_ops,
                  e->d_rules, e->d_tally_slots, e->d_tally_items, e->d_base_slots, e->d_sum_bases, e->d_sum_members, e->d_acc_sums, e->d_acc_members, e->d_defer_slots, e->d_blob, e->d_cpts, e->d_prefixes, e->d_key_words,
                  e->tally_saved, e->tally_saved2, e->tally_saved3, e->d_tally_enc, e->d_wire, e->d_status, e->gen_ws, e->d_gen_desc, e->d_h_srcs, e->d_h_words,
                  e->d_small_stages, e->d_small_levels, e->small_ws};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  for (auto& w : e->set) {
    void* sp[] = {w.pts, w.cmp, w.chal, w.states, w.flags, w.bad_item, w.btab, w.dpt, w.sacc, w.encw, w.partial, w.tally};
    for (void* p : sp) if (p) (void)hipFree(p);
    if (w.stream) (void)hipStreamDestroy(w.stream);
    if (w.done) (void)hipEventDestroy(w.done);
  }
  if (e->fork) (void)hipEventDestroy(e->fork);
  if (e->last_done) (void)hipEventDestroy(e->last_done);
  if (e->saved_ev) (void)hipEventDestroy(e->saved_ev);
  comb_table_free(e->d_tabK); comb_table_free(e->d_tabK_big);
  comb_table_free(e->d_tabH); comb_table_free(e->d_tabH_big);
  if (e->copy_stream) (void)hipStreamDestroy(e->copy_stream);
  if (e->json_ring) (void)hipHostFree(e->json_ring);
  if (e->json_status_ring) (void)hipHostFree(e->json_status_ring);
  for (hipStream_t st : e->json_ctl) if (st) (void)hipStreamDestroy(st);
  delete e;
}

static EngineBufs make_bufs(const Engine* e, int set, const void* d_ballots, u32 n, void* d_status) {
  const Engine::WorkSet& w = e->set[set];
  EngineBufs B;
  B.wire = reinterpret_cast<const u32*>(d_ballots);
  B.stride_words = (u32)(e->plan.stride / 4);
  B.n = n;
  B.cap = e->cap;
  B.pts = w.pts; B.cmp = w.cmp; B.chal = w.chal; B.states = w.states; B.flags = w.flags; B.bad_item = w.bad_item;
  B.status = reinterpret_cast<u32*>(d_status);
  B.tabG = e->use_big ? e->ctx->tabG_big : e->ctx->tabG; B.tabK = e->use_big ? e->d_tabK_big : e->d_tabK; B.cpts = e->d_cpts; B.prefixes = e->d_prefixes; B.blob = e->d_blob;
  // each set works in its own part of the context's per-lane workspace (the grids of its kernels are 1 / n_sets of msm_blocks)
  B.ws = e->ctx->ws + (size_t)set * (e->ctx->msm_blocks / e->n_sets) * WS_QUADS * NT;
  B.btab = w.btab;
  B.sacc = w.sacc;
  B.dpt = w.dpt;
  B.encw = w.encw;
  B.tabH = e->use_big ? e->d_tabH_big : e->d_tabH;
  return B;
}

// bytes of chunk workspace per ballot of ONE work set (the buffers engine_reserve allocates for it)
static size_t engine_bytes_per_ballot(const Engine* e) {
  const eghost::Plan& P = e->plan;
  const size_t pt = (size_t)PT_WORDS * sizeof(u32);
  return (size_t)std::max(P.n_pt_slots, 1) * pt + (size_t)std::max(P.n_cmp_slots, 1) * (32 + pt) + (size_t)std::max(P.n_chal_slots, 1) * 32 +
         (size_t)std::max(P.n_state_slots, 1) * 208 + (size_t)std::max(P.n_flag_slots, 1) * 4 + 4 +
         std::max<size_t>(P.n_tables(), 1) * btab_quads_of(e->teeth) * 16 + (size_t)std::max(e->max_defer, 1) * 2 * EG_NL * sizeof(u32) +
         (P.grouped() ? P.sum_bases.size() * (size_t)e->teeth * BTAB_ENTRY_QUADS * 16 : 0);
}

// (re)allocate the per-chunk SoA buffers of every work set for chunks of up to `want` ballots
static void engine_release_sets(Engine* e) {
  for (auto& w : e->set) {
    void** bufs[] = {(void**)&w.pts, (void**)&w.cmp, (void**)&w.chal, (void**)&w.states, (void**)&w.flags, (void**)&w.bad_item,
                     (void**)&w.btab, (void**)&w.dpt, (void**)&w.encw, (void**)&w.sacc};
    for (void** b : bufs) { if (*b) (void)hipFree(*b); *b = nullptr; }
  }
  e->cap = 0;
}
static int engine_reserve(Engine* e, u32 want) {
  if (want <= e->cap) return EG_OK;
  const eghost::Plan& P = e->plan;
  HIPCHK(hipDeviceSynchronize());   // earlier batches may still be running on a caller's stream
  engine_release_sets(e);
  const size_t cap = (want + NT - 1) / NT * NT;
  const size_t sizes[] = {(size_t)std::max(P.n_pt_slots, 1) * PT_QUADS * cap * sizeof(uint4),
                          (size_t)std::max(P.n_cmp_slots, 1) * 2 * cap * sizeof(uint4),
                          (size_t)std::max(P.n_chal_slots, 1) * 2 * cap * sizeof(uint4),
                          (size_t)std::max(P.n_state_slots, 1) * 52 * cap * sizeof(u32),
                          (size_t)std::max(P.n_flag_slots, 1) * cap * sizeof(u32),
                          cap * sizeof(u32),
                          std::max<size_t>(P.n_tables(), 1) * cap * btab_quads_of(e->teeth) * sizeof(uint4),
                          (size_t)std::max(P.n_cmp_slots, 1) * PT_QUADS * cap * sizeof(uint4),
                          (size_t)std::max(e->max_defer, 1) * 2 * EG_NL * cap * sizeof(u32),
                          P.grouped() ? std::max<size_t>(P.sum_bases.size(), 1) * cap * (size_t)e->teeth * BTAB_ENTRY_QUADS * sizeof(uint4) : (size_t)256};
  for (int k = 0; k < e->n_sets; ++k) {
    Engine::WorkSet& w = e->set[k];
    void** bufs[] = {(void**)&w.pts, (void**)&w.cmp, (void**)&w.chal, (void**)&w.states, (void**)&w.flags, (void**)&w.bad_item,
                     (void**)&w.btab, (void**)&w.dpt, (void**)&w.encw, (void**)&w.sacc};
    for (size_t i = 0; i < sizeof(sizes) / sizeof(sizes[0]); ++i) {
      const hipError_t he = hipMalloc(bufs[i], sizes[i]);
      if (he == hipErrorOutOfMemory) {        // the caller retries with smaller chunks
        (void)hipGetLastError();
        engine_release_sets(e);
        return fail(EG_ERR_NOMEM, "device memory exhausted while reserving the chunk workspace");
      }
      HIPCHK(he);
    }
  }
  e->cap = (u32)cap;
  return EG_OK;
}

static unsigned blocks_of(size_t n) { return (unsigned)std::max<size_t>(1, (n + NT - 1) / NT); }
static int grid_for(size_t lanes, int cap_blocks) {
  size_t blocks = (lanes + NT - 1) / NT;
  if (blocks < 1) blocks = 1;
  if ((size_t)cap_blocks < blocks) blocks = (size_t)cap_blocks;
  return (int)blocks;
}

// build device state for a plan + election key
// h: encoding of the third fixed base of a plan with H terms (Plan::h_srcs), null for every other plan
static int engine_create(eg_ctx* ctx, eghost::Plan&& plan, const uint8_t pk[32], int n_options, Engine** out, const uint8_t* h = nullptr) {
  std::unique_ptr<Engine, void (*)(Engine*)> e(new Engine(), engine_free);
  e->ctx = ctx;
  e->plan = std::move(plan);
  e->n_options = n_options;
  eghost::Plan& P = e->plan;
  hipStream_t s = ctx->stream;
  HIPCHK(hipSetDevice(ctx->device));
  if (P.pk_off >= 0) memcpy(P.blob.data() + P.pk_off, pk, 32);

  // flatten stages / levels / programs (pure host logic: host_plan.hpp)
  const eghost::FlatPlan F = eghost::flatten_plan(P);
  {
    const std::string why = eghost::check_flat_plan(P, F);
    if (!why.empty()) return fail(EG_ERR_BAD_ARG, "internal: inconsistent verification plan: " + why);
  }
  e->stages = F.stages;
  e->levels = F.levels;
  e->max_defer = F.max_defer;
  e->prefix_inst_first = F.prefix_inst_first;
  e->prefix_inst_count = F.prefix_inst_count;
  const std::vector<egplan::JobClass>& jobs = F.jobs;
  const std::vector<egplan::HashInst>& insts = F.insts;
  const std::vector<egplan::HashOp>& ops = F.ops;
  const std::vector<uint16_t>& defer_slots = F.defer_slots;
  const std::vector<egplan::DeriveClass>& dclasses = F.dclasses;
  int rc;
  if ((rc = upload(&e->d_pt_items, P.pt_items, s))) return rc;
  if ((rc = upload(&e->d_sc_items, P.sc_items, s))) return rc;
  if ((rc = upload(&e->d_dclasses, dclasses, s))) return rc;
  if ((rc = upload(&e->d_dterms, P.dterms, s))) return rc;
  if ((rc = upload(&e->d_jobs, jobs, s))) return rc;
  if ((rc = upload(&e->d_vterms, P.vterms, s))) return rc;
  if ((rc = upload(&e->d_insts, insts, s))) return rc;
  if ((rc = upload(&e->d_ops, ops, s))) return rc;
  if ((rc = upload(&e->d_rules, P.rules, s))) return rc;
  if ((rc = upload(&e->d_tally_slots, P.tally_slots, s))) return rc;
  {
    const std::vector<uint32_t> items = eggt::tally_items(P.pt_items, P.tally_slots);
    for (uint32_t it : items) if (it == 0xffffffffu) return fail(EG_ERR_BAD_ARG, "internal: a tally slot of the plan is not a wire point");
    if ((rc = upload(&e->d_tally_items, items, s))) return rc;
    std::vector<uint32_t> r_items;
    e->weed_keys_ok = egw::key_items(r_items, items) && P.stride % 16 == 0;
  }
  if ((rc = upload(&e->d_base_slots, F.build_slots, s))) return rc;
  if ((rc = upload(&e->d_sum_bases, F.sums, s))) return rc;
  if ((rc = upload(&e->d_sum_members, F.sum_members, s))) return rc;
  if ((rc = upload(&e->d_acc_sums, F.acc_sums, s))) return rc;
  if ((rc = upload(&e->d_acc_members, F.acc_members, s))) return rc;
  e->n_sums = (int)F.sums.size();
  if ((rc = upload(&e->d_defer_slots, defer_slots, s))) return rc;
  if ((rc = upload(&e->d_blob, P.blob, s))) return rc;
  if (P.has_h() != (h != nullptr)) return fail(EG_ERR_BAD_ARG, "internal: a plan has terms over a third fixed base exactly when one is given");
  if (P.has_h() && (rc = upload(&e->d_h_srcs, P.h_srcs, s))) return rc;

  // election key: decode, reject invalid / identity (keys/mod.rs:161-176), fixed-base table
  u32* d_pk = nullptr;
  u32* d_flags = nullptr;
  HIPCHK(hipMalloc((void**)&d_pk, 32));
  HIPCHK(hipMalloc((void**)&d_flags, 8));
  HIPCHK(hipMalloc((void**)&e->d_key_words, 2 * PT_WORDS * sizeof(u32)));
  HIPCHK(hipMemcpyAsync(d_pk, pk, 32, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_setup_points, dim3(1), dim3(64), 0, s, d_pk, e->d_key_words, d_flags);
  u32 hflags[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(hflags, d_flags, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  (void)hipFree(d_pk); (void)hipFree(d_flags);
  if (!hflags[0]) return fail(EG_ERR_BAD_PUBLIC_KEY, "public key is not a valid ristretto255 encoding");
  if (hflags[1]) return fail(EG_ERR_BAD_PUBLIC_KEY, "public key is the identity");
  if ((rc = comb_table_build(e->d_key_words + PT_WORDS, EG_COMB_BITS, s, &e->d_tabK))) return rc;
  if (h) {   // the third fixed base: decoded like the key; the identity is refused (its comb table is a case nothing here has ever built)
    HIPCHK(hipMalloc((void**)&d_pk, 32));
    HIPCHK(hipMalloc((void**)&d_flags, 8));
    HIPCHK(hipMalloc((void**)&e->d_h_words, 2 * PT_WORDS * sizeof(u32)));
    HIPCHK(hipMemcpyAsync(d_pk, h, 32, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_setup_points, dim3(1), dim3(64), 0, s, d_pk, e->d_h_words, d_flags);
    HIPCHK(hipMemcpyAsync(hflags, d_flags, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    (void)hipFree(d_pk); (void)hipFree(d_flags);
    if (!hflags[0]) return fail(EG_ERR_BAD_ARG, "blinding base is not a valid ristretto255 encoding");
    if (hflags[1]) return fail(EG_ERR_BAD_ARG, "blinding base is the identity");
    if ((rc = comb_table_build(e->d_h_words + PT_WORDS, EG_COMB_BITS, s, &e->d_tabH))) return rc;
  }

  // election-constant points [m]G
  {
    u64* d_m = nullptr;
    std::vector<uint64_t> mults = P.const_mults;
    if (mults.empty()) mults.push_back(0);
    HIPCHK(hipMalloc((void**)&d_m, mults.size() * 8));
    HIPCHK(hipMemcpyAsync(d_m, mults.data(), mults.size() * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMalloc((void**)&e->d_cpts, mults.size() * PT_QUADS * sizeof(uint4)));
    hipLaunchKernelGGL(k_const_points, dim3((unsigned)((mults.size() + NT - 1) / NT)), dim3(NT), 0, s, d_m, (int)mults.size(),
                       ctx->tabG, e->d_cpts);
    HIPCHK(hipStreamSynchronize(s));
    (void)hipFree(d_m);
  }

  // chunk workspace: sized lazily by engine_reserve() for the batches actually seen (up to EG_CHUNK ballots per chunk and work set)
  e->teeth = eghost::plan_teeth(e->plan);
  e->knobs = read_knobs();
  memcpy(e->key_bytes, pk, 32);
  if (e->knobs.teeth) e->teeth = e->knobs.teeth;     // measurement knob
  e->n_sets = e->knobs.streams;
  // k_encode_hash (kernels.cuh) needs one thing of a stage: at most 16 deferred commitments, since it encodes those of TWO ballots in
  // one batch of at most 32 (the bits of its zero_mask, the encw scratch rows).  It is switched on per PLAN, and more narrowly than the
  // kernel needs, on purpose: only for ballot plans (the ones that tally) ALL of whose stages fit, which is single choice with up to 7
  // options - the plans it was measured and tested on.  Multi-choice, quadratic voting and the proof plans (range, share, commitment
  // equivalence), which have no tally, keep k_encode_batch + k_hash in every stage even where one stage would fit, so that their
  // launches stay those of the profiles kept for them.  Within a fused plan a stage that defers nothing or hashes nothing (launch site
  // in engine_verify_device) also takes the two-kernel path, which then launches only the kernel that has work.
  e->fused_tail = !e->plan.tally_slots.empty();
  for (auto& st : e->stages)
    if (2 * st.defer_count > 32) e->fused_tail = false;
  // Two work sets whose kernels fill each other's launch tails (profiles/r03_ab_experiments.txt, blocks 3 and 9; M single-choice ballots/s):
  // with 6-tooth tables (57.6 KB per ballot and set) one set of 2^20 ballots 6.06, one set of 2^18 5.81 (-4 %), two sets of 2^18 6.05,
  // two sets of 2^19 6.13 (+1 %), two sets of 2^17 5.90; with the 5-tooth tables of the choice ballots (32.3 KB) two sets of 2^18 6.28,
  // of 2^19 6.35.  Default: two sets of 2^19 ballots where that stays within 40 GB (the choice ballots of up to ~6 options: 34 GB),
  // else of 2^18 (16 options: 44 GB; quadratic voting 5 / 20: 42 GB); EG_CHUNK overrides.
  {
    const size_t per = engine_bytes_per_ballot(e.get()) * (size_t)e->n_sets;
    const u32 two_sets = per * 524288u <= ((size_t)40 << 30) ? 524288u : 262144u;
    e->max_cap = e->knobs.chunk ? (u32)std::min<size_t>(e->knobs.chunk, 1u << 30) : (e->n_sets == 2 ? two_sets : 1048576u);
  }
  {
    // Large elections keep the workspace within half of the free device memory (~58 KB per ballot and set for 5 options, 150 KB for 16).
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const size_t per = engine_bytes_per_ballot(e.get()) * (size_t)e->n_sets;
    const size_t limit = per ? free_b / 2 / per : e->max_cap;
    if (limit < e->max_cap) e->max_cap = (u32)(limit / NT * NT);
  }
  if (e->max_cap < NT) e->max_cap = NT;
  e->max_cap = (e->max_cap + NT - 1) / NT * NT;
  const size_t tally_bytes = std::max<size_t>(P.tally_slots.size(), 1) * PT_WORDS * sizeof(u32);
  for (int k = 0; k < e->n_sets; ++k) {
    Engine::WorkSet& w = e->set[k];
    HIPCHK(hipMalloc((void**)&w.partial, tally_bytes * e->tally_blocks));
    HIPCHK(hipMalloc((void**)&w.tally, tally_bytes));
    hipLaunchKernelGGL(k_tally_init, dim3(blocks_of(P.tally_slots.size())), dim3(NT), 0, s, w.tally, (int)P.tally_slots.size());
    if (e->n_sets > 1) {
      HIPCHK(hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
      HIPCHK(hipEventCreateWithFlags(&w.done, hipEventDisableTiming));
    }
  }
  if (e->n_sets > 1) HIPCHK(hipEventCreateWithFlags(&e->fork, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&e->last_done, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&e->saved_ev, hipEventDisableTiming));
  e->tally = e->set[0].tally;
  HIPCHK(hipMalloc((void**)&e->tally_saved, tally_bytes));
  HIPCHK(hipMalloc((void**)&e->tally_saved2, tally_bytes));
  HIPCHK(hipMalloc((void**)&e->tally_saved3, tally_bytes));
  HIPCHK(hipMalloc((void**)&e->d_tally_enc, std::max<size_t>(P.tally_slots.size(), 1) * 32));
  HIPCHK(hipMalloc((void**)&e->d_prefixes, (size_t)std::max(P.n_prefixes, 1) * 52 * sizeof(u32)));

  // hoisted transcript prefixes: run the prefix programs once (a single lane each)
  if (e->prefix_inst_count) {
    EngineBufs B = make_bufs(e.get(), 0, nullptr, 1, nullptr);
    hipLaunchKernelGGL(k_hash, dim3(grid_for(e->prefix_inst_count, 1 << 20)), dim3(NT), 0, s, B, e->d_insts, e->d_ops,
                       e->prefix_inst_first, e->prefix_inst_count);
  }
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipGetLastError());
  *out = e.release();
  ctx->refs.fetch_add(1);   // dropped by params_destroy
  return EG_OK;
}

// Wide comb tables for G (per context) and K (per engine): built when an engine has seen ctx->big_min items (in one batch or over
// many calls: a host batch arrives in pieces, JSON text window by window), kept for the life of the objects.  A table that does not fit the device memory is not an error: the narrow tables stay in use.
static int ensure_big_tables(Engine* e, hipStream_t s) {
  eg_ctx* ctx = e->ctx;
  if (ctx->big_bits == 0 || ctx->big_failed) return EG_OK;
  if (!ctx->tabG_big) {
    const int rc = comb_table_build(ctx->gen_words, ctx->big_bits, s, &ctx->tabG_big, true);
    if (rc == EG_ERR_NOMEM) { ctx->big_failed = true; return EG_OK; }
    if (rc) return rc;
  }
  if (!e->d_tabK_big) {
    const int rc = comb_table_build(e->d_key_words + PT_WORDS, ctx->big_bits, s, &e->d_tabK_big, true);
    if (rc == EG_ERR_NOMEM) { ctx->big_failed = true; return EG_OK; }
    if (rc) return rc;
  }
  if (e->d_tabH && !e->d_tabH_big) {     // a third base goes wide with the other two, or all three stay narrow (engine_wide)
    const int rc = comb_table_build(e->d_h_words + PT_WORDS, ctx->big_bits, s, &e->d_tabH_big, true);
    if (rc == EG_ERR_NOMEM) { ctx->big_failed = true; return EG_OK; }
    if (rc) return rc;
  }
  return EG_OK;
}
// one launch reads one width: the wide tables only when every fixed base of the engine has one
static bool engine_wide(const Engine* e) {
  return e->d_tabK_big != nullptr && e->ctx->tabG_big != nullptr && (e->d_tabH == nullptr || e->d_tabH_big != nullptr);
}

// the kernels that touch the per-ballot comb tables exist once per comb shape (template parameter T, ge25519.cuh: Teeth<T>)
#ifdef EG_TEETH7      // measurement builds only (tools/build_variant.sh teeth7 -DEG_TEETH7): the 7 x 37 comb (64 entries, 8 KiB per table) as a third shape
#define EG_WITH_TEETH(teeth, ...) do { if ((teeth) == 5) { constexpr int T = 5; __VA_ARGS__; } else if ((teeth) == 7) { constexpr int T = 7; __VA_ARGS__; } else { constexpr int T = 6; __VA_ARGS__; } } while (0)
#else
#define EG_WITH_TEETH(teeth, ...) do { if ((teeth) == 5) { constexpr int T = 5; __VA_ARGS__; } else { constexpr int T = 6; __VA_ARGS__; } } while (0)
#endif

// marks the end of an asynchronous call that touched the engine's running tally on stream s (Engine::last_done)
static int engine_touch(Engine* e, hipStream_t s) {
  HIPCHK(hipEventRecord(e->last_done, s));
  e->last_used = true;
  return EG_OK;
}
// verify n ballots (device pointers), accumulating accepted ciphertexts into the running tally
// flags (the streaming JSON entry points overlap consecutive calls on different control streams `s`):
//   VD_FORCE_SETS     always run on the work sets' own streams (never on `s` with set 0's buffers), whatever the size of the batch;
//   VD_KEEP_SET_TALLY leave set 1's share of the tally in its accumulator at the join (the caller merges once, when everything has landed).
enum { VD_FORCE_SETS = 1, VD_KEEP_SET_TALLY = 2 };
static int engine_verify_device(Engine* e, size_t n, const void* d_ballots, void* d_status, hipStream_t s, int flags = 0) {
  eg_ctx* ctx = e->ctx;     // s may be the null stream: a NULL hipStream_t means what it means everywhere in HIP
  const eghost::Plan& P = e->plan;
  size_t all_idx = 0;
  int rc;
  e->items_seen += n;
  if (e->items_seen >= ctx->big_min && (rc = ensure_big_tables(e, s))) return rc;
  e->use_big = engine_wide(e);
  if ((rc = prof_begin(ctx, s, PROF_CALL, &all_idx))) return rc;
  // equal-sized chunks (each a multiple of the block size) so that the persistent grids stay balanced on the last chunk; with two
  // work sets a batch that is worth splitting gets an even number of chunks, so that both streams carry the same load
  const bool two = e->n_sets == 2 && ((flags & VD_FORCE_SETS) || (n >= (size_t)ctx->resident_blocks * NT / 2 && !ctx->prof_serial));
  auto chunks_for = [&](size_t cap) {
    size_t k = (n + cap - 1) / cap;
    if (two) k = std::max<size_t>(2, (k + 1) / 2 * 2);
    return k;
  };
  size_t n_chunks = chunks_for(e->max_cap);
  while (n) {
    const int rr = engine_reserve(e, (u32)(((n + n_chunks - 1) / n_chunks + NT - 1) / NT * NT));
    if (rr == EG_OK) break;
    if (rr != EG_ERR_NOMEM || e->max_cap <= 16 * NT) return rr;
    e->max_cap = (e->max_cap / 2 + NT - 1) / NT * NT;    // other allocations took the memory this engine counted on: halve the chunks
    n_chunks = chunks_for(e->max_cap);
  }
  const size_t even = n_chunks ? ((n + n_chunks - 1) / n_chunks + NT - 1) / NT * NT : 0;
  // join: the caller's stream continues after both sets; set 1's share of the tally moves into the running tally.  It runs on EVERY
  // way out once the sets have been forked (the scope guard below): an early return between fork and join (a failed launch, event or
  // allocation) used to leave the caller's stream ahead of work still queued on the sets' streams - the caller would then free or
  // re-use buffers those kernels still write, and set 1's accumulator would carry a stale share into the next call.
  bool forked = false, joined = false;
  auto join = [&]() -> hipError_t {
    joined = true;
    hipError_t first = hipSuccess;
    for (int k = 0; k < 2; ++k) {
      if (ws_release(ctx, 1u << k, e->set[k].stream) != EG_OK && first == hipSuccess) first = hipErrorUnknown;   // the next user of this half waits for it
      hipError_t he = hipEventRecord(e->set[k].done, e->set[k].stream);
      if (he == hipSuccess) he = hipStreamWaitEvent(s, e->set[k].done, 0);
      if (he != hipSuccess && first == hipSuccess) first = he;
    }
    const int ns = (int)P.tally_slots.size();
    if (ns && !(flags & VD_KEEP_SET_TALLY)) {
      hipLaunchKernelGGL(k_tally_add_points, dim3(blocks_of((size_t)ns)), dim3(NT), 0, s, e->set[1].tally, ns, e->set[0].tally);
      hipLaunchKernelGGL(k_tally_init, dim3(blocks_of((size_t)ns)), dim3(NT), 0, s, e->set[1].tally, ns);
    }
    return first;
  };
  ScopeExit rejoin{[&]() {
    if (!forked || joined) return;
    if (join() != hipSuccess) (void)hipDeviceSynchronize();     // the streams could not even be tied together: drain the device instead
  }};
  bool whole_ws = false;       // a one-set call holds both halves of the context's per-lane workspace on `s` until it returns
  ScopeExit release_ws{[&]() { if (whole_ws) (void)ws_release(ctx, 3u, s); }};
  if (two) {                 // fork: both work sets start after whatever the caller's stream holds so far
    HIPCHK(hipEventRecord(e->fork, s));
    forked = true;
    for (int k = 0; k < 2; ++k) {
      HIPCHK(hipStreamWaitEvent(e->set[k].stream, e->fork, 0));
      TRY_(ws_acquire(ctx, 1u << k, e->set[k].stream));      // ... and after the last user of its half of the workspace, whoever that was
    }
  } else if (n) {
    TRY_(ws_acquire(ctx, 3u, s));
    whole_ws = true;
  }
  const bool inject_failure = two && EG_FAULT_POINT(after_fork);     // constant false in the shipped library (see EG_FAULT_POINT above)
  const int msm_blocks = ctx->msm_blocks / (two ? 2 : 1);
  size_t chunk = 0;
  for (size_t off = 0; off < n; off += even, ++chunk) {
    const int set = two ? (int)(chunk & 1) : 0;
    hipStream_t cs = two ? e->set[set].stream : s;
    const Engine::WorkSet& w = e->set[set];
    const u32 cn = (u32)std::min<size_t>(even, n - off);
    EngineBufs B = make_bufs(e, set, reinterpret_cast<const unsigned char*>(d_ballots) + off * P.stride, cn,
                             reinterpret_cast<u32*>(d_status) + off);
    if (!two) B.ws = ctx->ws;
    const int wide = ctx->cus * 32;     // grid-stride kernels that need no per-lane workspace: well oversubscribed (see eg_init)
    HIPCHK(hipMemsetAsync(w.bad_item, 0xff, (size_t)cn * sizeof(u32), cs));
    hipLaunchKernelGGL(k_decode_points, dim3(grid_for((size_t)P.pt_items.size() * cn, wide)), dim3(NT), 0, cs, B, e->d_pt_items,
                       (int)P.pt_items.size());
    hipLaunchKernelGGL(k_check_scalars, dim3(grid_for((size_t)P.sc_items.size() * cn, wide)), dim3(NT), 0, cs, B, e->d_sc_items,
                       (int)P.sc_items.size());
    for (auto& lv : e->levels)
      if (lv.count)
        hipLaunchKernelGGL(k_derive_points, dim3(grid_for((size_t)lv.count * cn, wide)), dim3(NT), 0, cs, B, e->d_dclasses,
                           e->d_dterms, lv.first, lv.count);
    for (auto& st : e->stages) {
      // the comb tables this stage starts with (host_plan.hpp: Stage): every table of the ballot before stage 0, or - ring-group walk -
      // the tables of one group of rings in the table slots the previous group has finished with
      if (st.build_count) {
        size_t pi = 0;
        if ((rc = prof_begin(ctx, cs, PROF_TABLES, &pi))) return rc;
        EG_WITH_TEETH(e->teeth, hipLaunchKernelGGL(k_base_tables<T>, dim3(grid_for((size_t)st.build_count * cn, msm_blocks)), dim3(NT), 0, cs, B,
                                                   e->d_base_slots + st.build_first, st.build_count));
        if ((rc = prof_end(ctx, cs, pi))) return rc;
      }
      if (st.sums_direct)
        EG_WITH_TEETH(e->teeth, hipLaunchKernelGGL(k_sum_tables<T>, dim3(grid_for((size_t)e->n_sums * cn, msm_blocks)), dim3(NT), 0, cs, B,
                                                   e->d_sum_bases, e->d_sum_members, e->n_sums));
      if (st.acc_count)
        EG_WITH_TEETH(e->teeth, hipLaunchKernelGGL(k_sum_accumulate<T>, dim3(grid_for((size_t)st.acc_count * T * cn, msm_blocks)), dim3(NT), 0, cs, B,
                                                   e->d_acc_sums + st.acc_first, e->d_acc_members, st.acc_count));
      if (st.sum_finish)
        EG_WITH_TEETH(e->teeth, hipLaunchKernelGGL(k_sum_finish<T>, dim3(grid_for((size_t)e->n_sums * cn, msm_blocks)), dim3(NT), 0, cs, B,
                                                   e->d_sum_bases, e->n_sums));
      if (st.fam_count[FAM_TABLE1]) {
        size_t pi = 0;
        if ((rc = prof_begin(ctx, cs, PROF_MSM, &pi))) return rc;
        EG_WITH_TEETH(e->teeth, hipLaunchKernelGGL((k_eq_table<false, T>), dim3(grid_for((size_t)st.fam_count[FAM_TABLE1] * cn, msm_blocks)), dim3(NT), 0, cs,
                                                   B, e->d_jobs, e->d_vterms, st.fam_first[FAM_TABLE1], st.fam_count[FAM_TABLE1], 1));
        if ((rc = prof_end(ctx, cs, pi))) return rc;
      }
      if (st.fam_count[FAM_TABLEN]) {
        const int group = std::min(st.max_terms, EG_MULTI_GROUP);
        EG_WITH_TEETH(e->teeth, hipLaunchKernelGGL((k_eq_table<true, T>), dim3(grid_for((size_t)st.fam_count[FAM_TABLEN] * cn, msm_blocks)), dim3(NT),
                                                   (size_t)group * 9 * NT * sizeof(u32), cs, B, e->d_jobs, e->d_vterms, st.fam_first[FAM_TABLEN],
                                                   st.fam_count[FAM_TABLEN], group));
      }
      if (st.fam_count[FAM_DIRECT1] && e->d_tabH)       // a plan with a third fixed base: the kernel that also reads the table of H
        hipLaunchKernelGGL(k_eq_direct_h, dim3(grid_for((size_t)st.fam_count[FAM_DIRECT1] * cn, msm_blocks)), dim3(NT), 0, cs, B,
                           e->d_jobs, e->d_vterms, e->d_h_srcs, st.fam_first[FAM_DIRECT1], st.fam_count[FAM_DIRECT1]);
      else if (st.fam_count[FAM_DIRECT1])
        hipLaunchKernelGGL(k_eq_direct, dim3(grid_for((size_t)st.fam_count[FAM_DIRECT1] * cn, msm_blocks)), dim3(NT), 0, cs, B,
                           e->d_jobs, e->d_vterms, st.fam_first[FAM_DIRECT1], st.fam_count[FAM_DIRECT1]);
      if (st.fam_count[FAM_GENERIC])
        EG_WITH_TEETH(e->teeth, hipLaunchKernelGGL(k_eq_generic<T>, dim3(grid_for((size_t)st.fam_count[FAM_GENERIC] * cn, msm_blocks)), dim3(NT), 0, cs, B,
                           e->d_jobs, e->d_vterms, st.fam_first[FAM_GENERIC], st.fam_count[FAM_GENERIC]));
      if (st.fam_count[FAM_ENCODE])
        hipLaunchKernelGGL(k_encode_plain, dim3(grid_for((size_t)st.fam_count[FAM_ENCODE] * cn, wide)), dim3(NT), 0, cs, B, e->d_jobs,
                           st.fam_first[FAM_ENCODE], st.fam_count[FAM_ENCODE]);
      // the stage's tail in one launch: two ballots a lane, one inversion a pair
      if (e->fused_tail && st.inst_count && st.defer_count) {
        if (2 * st.defer_count > 32) return fail(EG_ERR_BAD_ARG, "internal: a stage of a fused plan defers more than 16 commitments");
        hipLaunchKernelGGL(k_encode_hash, dim3(blocks_of(((size_t)cn + 1) / 2)), dim3(NT), 0, cs, B, e->d_defer_slots + st.defer_first,
                           st.defer_count, e->d_insts, e->d_ops, st.inst_first, st.inst_count);
        continue;
      }
      for (int d0 = 0; d0 < st.defer_count; d0 += 32)   // one batched inversion per ballot and group of <= 32 commitments
        hipLaunchKernelGGL(k_encode_batch, dim3(grid_for(cn, wide)), dim3(NT), 0, cs, B, e->d_defer_slots + st.defer_first + d0,
                           std::min(32, st.defer_count - d0));
      if (st.inst_count)
        hipLaunchKernelGGL(k_hash, dim3(grid_for((size_t)st.inst_count * cn, 1 << 30)), dim3(NT), 0, cs, B, e->d_insts, e->d_ops,
                           st.inst_first, st.inst_count);
    }
    hipLaunchKernelGGL(k_status, dim3((cn + NT - 1) / NT), dim3(NT), 0, cs, B, e->d_rules, (int)P.rules.size());
    if (inject_failure && chunk == 0) return fail(EG_ERR_HIP, "injected failure between fork and join (fault point of a test build)");
    if (P.tally_slots.empty()) continue;
    const int G = std::min<int>(e->tally_blocks, (int)((cn + NT - 1) / NT));
    hipLaunchKernelGGL(k_tally_partial, dim3(G, (unsigned)P.tally_slots.size()), dim3(NT), 0, cs, B, e->d_tally_slots, w.partial);
    hipLaunchKernelGGL(k_tally_final, dim3((unsigned)P.tally_slots.size()), dim3(NT), 0, cs, w.partial, G, w.tally);
  }
  if (two) HIPCHK(join());
  if ((rc = prof_end(ctx, s, all_idx))) return rc;
  if ((rc = engine_touch(e, s))) return rc;
  HIPCHK(hipGetLastError());
  return EG_OK;
}

// ---- the small-batch path: one launch of k_ballot_small (one workgroup per ballot, latency_kernels.cuh), then the batch path's tally ----
// Same contract as engine_verify_device for n <= EG_SMALL_BATCH_MAX: verdicts in d_status, accepted ballots added to the running tally.
// It works in work set 0 like a one-set batch call, so it takes both halves of the context's workspace protocol: calls of either
// kind on one params object are then ordered on the GPU whatever streams they use.  The narrow comb tables are read always (a
// handful of ballots does not pay for the wide ones), and every comb table of a ballot is resident whatever ring-group walk the
// plan was built with - the walk's table slots are re-used stage by stage exactly as the batch path re-uses them.
static int engine_small_prepare(Engine* e, size_t n, hipStream_t s) {
  if (!e->small_threads) {
    // k_ballot_small has no counterpart of k_eq_direct_h: an equation with a term over the third fixed base H would come out without it
    if (e->plan.has_h()) return fail(EG_ERR_BAD_ARG, "internal: the small-batch path does not evaluate terms over a third fixed base");
    int quads = 1;
    bool needs_ws = false;
    for (auto& st : e->stages) {
      quads = std::max(quads, std::max(st.build_count, st.fam_count[FAM_TABLE1]));
      if (st.fam_count[FAM_DIRECT1] || st.fam_count[FAM_GENERIC]) needs_ws = true;
    }
    int rc;
    if ((rc = upload(&e->d_small_stages, e->stages, s))) return rc;
    if ((rc = upload(&e->d_small_levels, e->levels, s))) return rc;
    e->small_needs_ws = needs_ws;
    e->small_threads = std::min(SM_MAX_THREADS, std::max(64, (quads * 4 + 63) / 64 * 64));
  }
  if (e->small_needs_ws && n > e->small_ws_ballots) {
    HIPCHK(hipDeviceSynchronize());     // an earlier small call may still use the old slice
    if (e->small_ws) (void)hipFree(e->small_ws);
    e->small_ws = nullptr; e->small_ws_ballots = 0;
    size_t cap = 64;
    while (cap < n) cap *= 2;
    HIPCHK(hipMalloc((void**)&e->small_ws, cap * SM_LANES * WS_QUADS * sizeof(uint4)));
    e->small_ws_ballots = cap;
  }
  return EG_OK;
}
static int engine_verify_small_device(Engine* e, size_t n, const void* d_ballots, void* d_status, hipStream_t s) {
  eg_ctx* ctx = e->ctx;
  const eghost::Plan& P = e->plan;
  if (!n) return EG_OK;
  int rc;
  if ((rc = engine_small_prepare(e, n, s))) return rc;
  if ((rc = engine_reserve(e, (u32)((n + NT - 1) / NT * NT)))) return rc;
  size_t all_idx = 0;
  if ((rc = prof_begin(ctx, s, PROF_CALL, &all_idx))) return rc;
  TRY_(ws_acquire(ctx, 3u, s));
  ScopeExit release_ws{[&]() { (void)ws_release(ctx, 3u, s); }};
  const Engine::WorkSet& w = e->set[0];
  EngineBufs B = make_bufs(e, 0, d_ballots, (u32)n, d_status);
  B.tabG = ctx->tabG; B.tabK = e->d_tabK; B.tabH = e->d_tabH;
  SmallPlanDev D;
  D.pt_items = e->d_pt_items; D.sc_items = e->d_sc_items; D.n_pt = (int)P.pt_items.size(); D.n_sc = (int)P.sc_items.size();
  D.dclasses = e->d_dclasses; D.dterms = e->d_dterms;
  D.levels = e->d_small_levels; D.n_levels = (int)e->levels.size();
  D.stages = e->d_small_stages; D.n_stages = (int)e->stages.size();
  D.jobs = e->d_jobs; D.vterms = e->d_vterms; D.insts = e->d_insts; D.ops = e->d_ops;
  D.rules = e->d_rules; D.n_rules = (int)P.rules.size();
  D.base_slots = e->d_base_slots;
  D.sums = e->d_sum_bases; D.sum_members = e->d_sum_members; D.n_sums = e->n_sums;
  D.acc_sums = e->d_acc_sums; D.acc_members = e->d_acc_members;
  D.defer_slots = e->d_defer_slots;
  D.ws = e->small_ws;
  EG_WITH_TEETH(e->teeth, hipLaunchKernelGGL(k_ballot_small<T>, dim3((unsigned)n), dim3(e->small_threads), 0, s, B, D));
  if (!P.tally_slots.empty()) {
    const int G = std::min<int>(e->tally_blocks, (int)((n + NT - 1) / NT));
    hipLaunchKernelGGL(k_tally_partial, dim3(G, (unsigned)P.tally_slots.size()), dim3(NT), 0, s, B, e->d_tally_slots, w.partial);
    hipLaunchKernelGGL(k_tally_final, dim3((unsigned)P.tally_slots.size()), dim3(NT), 0, s, w.partial, G, w.tally);
  }
  if ((rc = prof_end(ctx, s, all_idx))) return rc;
  if ((rc = engine_touch(e, s))) return rc;
  HIPCHK(hipGetLastError());
  return EG_OK;
}

// encodes a tally held in device memory (the running tally, or a snapshot of it) into host bytes
static int engine_tally_encode_from(Engine* e, const u32* d_tally, uint8_t* out, bool drain_device = true) {
  hipStream_t s = e->ctx->stream;
  if (drain_device) HIPCHK(hipDeviceSynchronize());   // batches enqueued on caller streams by the _device entry points must have landed
  else if (e->last_used) HIPCHK(hipStreamWaitEvent(s, e->last_done, 0));      // (a caller that knows its streams have been waited for: only the engine's last call)
  const int ns = (int)e->plan.tally_slots.size();
  if (!ns) return EG_OK;
  hipLaunchKernelGGL(k_tally_encode, dim3(blocks_of((size_t)ns)), dim3(NT), 0, s, d_tally, ns, e->d_tally_enc);
  HIPCHK(hipMemcpyAsync(out, e->d_tally_enc, (size_t)ns * 32, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return EG_OK;
}
static int engine_tally_encode(Engine* e, uint8_t* out) { return engine_tally_encode_from(e, e->tally, out); }

// running tally += the points encoded in `in` (n_slots x 32 bytes): checkpoint / resume and merging of earlier batches
static int engine_tally_add(Engine* e, const uint8_t* in) {
  hipStream_t s = e->ctx->stream;
  HIPCHK(hipDeviceSynchronize());
  const int ns = (int)e->plan.tally_slots.size();
  u32* d_in = nullptr;
  HIPCHK(hipMalloc((void**)&d_in, (size_t)ns * 32 + 4));
  u32* d_bad = d_in + (size_t)ns * 8;
  HIPCHK(hipMemsetAsync(d_bad, 0, 4, s));
  HIPCHK(hipMemcpyAsync(d_in, in, (size_t)ns * 32, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_tally_add_encoded, dim3(blocks_of((size_t)ns)), dim3(NT), 0, s, d_in, ns, e->tally, d_bad);
  u32 bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  (void)hipFree(d_in);
  return bad ? fail(EG_ERR_BAD_ARG, "tally contains an invalid ristretto255 encoding") : EG_OK;
}

// device-side staging of the host forms: room for n packed ballots and their verdicts
static int engine_stage_reserve(Engine* e, size_t n) {
  if (n <= e->staging_ballots) return EG_OK;
  if (e->d_wire) (void)hipFree(e->d_wire);
  if (e->d_status) (void)hipFree(e->d_status);
  e->d_wire = nullptr; e->d_status = nullptr; e->staging_ballots = 0;
  HIPCHK(hipMalloc((void**)&e->d_wire, std::max<size_t>(n, 1) * e->plan.stride));
  HIPCHK(hipMalloc((void**)&e->d_status, std::max<size_t>(n, 1) * sizeof(u32)));
  e->staging_ballots = n;
  return EG_OK;
}

static int engine_verify_host(Engine* e, size_t n, const uint8_t* ballots, uint32_t* status, uint8_t* tally_out, bool small = false) {
  hipStream_t s = e->ctx->stream;
  HIPCHK(hipSetDevice(e->ctx->device));
  // The host form runs on the context's own stream but shares the engine's workspaces and running tally with whatever
  // `_device` calls enqueued on caller streams: wait for them, like the other host forms do.
  HIPCHK(hipDeviceSynchronize());
  const int ns = (int)e->plan.tally_slots.size();
  { const int rc = engine_stage_reserve(e, n); if (rc) return rc; }
  // fallible set-up comes BEFORE the running tally is set aside, and a scope guard puts it back on EVERY exit path (round 2 merged it
  // only on the explicit error paths: an early HIPCHK return in between lost the running tally)
  if (n && !e->copy_stream) HIPCHK(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
  // tally_out is the tally of THIS batch; the running tally keeps accumulating across calls (only eg_*_tally_reset clears
  // it).  The running tally is set aside, the batch is tallied from the identity, and the two are merged afterwards.
  bool set_aside = false;
  ScopeExit restore{[&]() {   // running tally = saved + this batch
    if (!set_aside) return;
    hipLaunchKernelGGL(k_tally_add_points, dim3(blocks_of((size_t)ns)), dim3(NT), 0, s, e->tally_saved, ns, e->tally);
    (void)hipStreamSynchronize(s);
  }};
  if (tally_out && ns) {
    HIPCHK(hipMemcpyAsync(e->tally_saved, e->tally, (size_t)ns * PT_WORDS * sizeof(u32), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_tally_init, dim3(blocks_of((size_t)ns)), dim3(NT), 0, s, e->tally, ns);
    set_aside = true;
  }
  if (n && !small && e->items_seen + n >= e->ctx->big_min) {     // the whole batch counts: its first piece already reads the wide comb tables
    const int rc = ensure_big_tables(e, s);
    if (rc) return rc;
  }
  if (n) {
    // Pipeline: the copy stream uploads piece k+1 while piece k is verified (host staging, not the kernels, is
    // the scaling risk when ballots arrive in host memory).  The first piece is small so that the exposed upload is short;
    // the rest are as large as the engine's chunks (large chunks waste less of each kernel's last round).
    std::vector<std::pair<size_t, size_t>> pieces;   // (offset, count)
    {
      const size_t lanes = (size_t)e->ctx->resident_blocks * NT;
      size_t off = 0;
      if (n >= lanes) {       // (a quarter of a mid-sized batch: 262 144 ballots +5 %, 131 072 +2.5 % over uploading them whole; below that the split costs more)
        const size_t f = std::min(lanes, (n / 4 + NT - 1) / NT * NT);
        pieces.push_back({0, f}); off = f;
      }
      const size_t piece_cap = (size_t)e->max_cap * e->n_sets;      // one piece = one chunk per work set
      const size_t rem = n - off, k = (rem + piece_cap - 1) / piece_cap;
      const size_t even = ((rem + k - 1) / k + NT - 1) / NT * NT;
      for (; off < n; off += even) pieces.push_back({off, std::min(even, n - off)});
    }
    std::vector<hipEvent_t> uploaded(pieces.size(), nullptr);
    size_t largest = 0;
    for (auto& pc : pieces) largest = std::max(largest, pc.second);
    int rc = engine_reserve(e, (u32)std::min<size_t>((largest + e->n_sets - 1) / e->n_sets + NT, e->max_cap));   // no regrowth of the workspace mid-pipeline
    if (rc == EG_ERR_NOMEM) rc = EG_OK;                // engine_verify_device falls back to smaller chunks
    for (size_t k = 0; k < pieces.size() && rc == EG_OK; ++k) {
      const size_t off = pieces[k].first, m = pieces[k].second;
      hipError_t he = hipEventCreateWithFlags(&uploaded[k], hipEventDisableTiming);
      if (he == hipSuccess) he = hipMemcpyAsync(e->d_wire + off * e->plan.stride, ballots + off * e->plan.stride, m * e->plan.stride,
                                                hipMemcpyHostToDevice, e->copy_stream);
      if (he == hipSuccess) he = hipEventRecord(uploaded[k], e->copy_stream);
      if (he == hipSuccess) he = hipStreamWaitEvent(s, uploaded[k], 0);
      if (he != hipSuccess) { rc = fail(EG_ERR_HIP, std::string("host upload: ") + hipGetErrorString(he)); break; }
      rc = small ? engine_verify_small_device(e, m, e->d_wire + off * e->plan.stride, e->d_status + off, s)
                 : engine_verify_device(e, m, e->d_wire + off * e->plan.stride, e->d_status + off, s);
    }
    // one download at the end: a device-to-pageable copy would stall the host (and the next upload) behind chunk k
    if (rc == EG_OK && hipMemcpyAsync(status, e->d_status, n * sizeof(u32), hipMemcpyDeviceToHost, s) != hipSuccess)
      rc = fail(EG_ERR_HIP, "status download failed");
    (void)hipStreamSynchronize(e->copy_stream);
    (void)hipStreamSynchronize(s);
    for (hipEvent_t ev : uploaded) if (ev) (void)hipEventDestroy(ev);
    if (rc) return rc;
  }
  HIPCHK(hipStreamSynchronize(s));
  if (tally_out) return engine_tally_encode(e, tally_out);      // (the guard merges the running tally back after the encoding)
  return EG_OK;
}

// ---------------------------------------------------------------------------------------------------------------
struct eg_choice_params { Engine* eng; int n_options; int single; };
struct eg_qv_params { Engine* eng; int n_options; uint64_t credits; eghost::QvShape shape; };
struct eg_proof_params {
  Engine* eng; int kind; size_t item_size;
  // what the provers need beyond the plan: the decomposition of a range proof (bool: one ring over [O, G]) and the values of a sum of squares
  uint64_t upper_bound = 0; eghost::RangeDecomposition range; int n_values = 0;
};
// between eg_verify_*_json_begin and eg_verify_json_end / _abort the params object belongs to the stream: its work sets, staging ring and
// running tally are in use, so every other verify / tally call on it is refused
static int refuse_if_streaming(const Engine* e) {
  return e->stream_open ? fail(EG_ERR_BAD_ARG, "a JSON stream is open on this params object (eg_verify_json_end or _abort it first)") : EG_OK;
}
void eg_verify_json_abort(struct eg_json_stream* S);
static bool stream_is_one_shot(const struct eg_json_stream* S);
// A LONG call (Engine::long_call_mu) - a one-shot JSON call (eg_verify_*_json: its worker thread takes the context's lock piece by piece) or a
// multi-GPU call (eg_verify_*_batch_multi*: one host thread per slab) - does not hold the context's lock for its length, but it is still
// ONE call on the params object as far as other threads are concerned: their calls on that object wait for it, as they would for any other
// entry point (the long call holds the engine's long_call_mu from start to end; the waiter drops the context's lock, queues on that mutex,
// takes the lock again and looks again).  An explicitly opened stream is the caller's own doing: calls are refused.
// (lk_ is the unique_lock of EG_LOCK / EG_LOCK_P in the calling entry point.)
#define EG_WAIT_LONG_ONLY(e)                                                                     \
  do {                                                                                           \
    while (((e)->stream_open && stream_is_one_shot((e)->stream_open)) || (e)->reserved) {        \
      lk_.unlock();                                                                              \
      { std::lock_guard<std::mutex> wait_((e)->long_call_mu); }                                  \
      lk_.lock();                                                                                \
    }                                                                                            \
  } while (0)
#define EG_WAIT_JSON(e)                                                                          \
  do {                                                                                           \
    EG_WAIT_LONG_ONLY(e);                                                                        \
    TRY(refuse_if_streaming(e));                                                                 \
  } while (0)

// The context is reference counted: the caller holds one reference (dropped by eg_destroy) and every params object
// created on it holds another, so params may be destroyed after the context they were created on.
static void ctx_release(eg_ctx* c) {
  if (!c || c->refs.fetch_sub(1) != 1) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (auto& sp : c->spans) { (void)hipEventDestroy(sp.a); (void)hipEventDestroy(sp.b); }
  for (auto& ev : c->event_pool) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : c->ws_done) if (ev) (void)hipEventDestroy(ev);
  comb_table_free(c->tabG); comb_table_free(c->tabG_big);
  if (c->gen_words) (void)hipFree(c->gen_words);
  if (c->ws) (void)hipFree(c->ws);
  if (c->prim_scratch) (void)hipFree(c->prim_scratch);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}
// destroys a params object: its engine under the context lock, then its reference on the context
template <class Params>
static void params_destroy(Params* p) {
  if (!p) return;
  eg_ctx* c = p->eng->ctx;
  if (p->eng->stream_open) eg_verify_json_abort(p->eng->stream_open);      // a stream left open dies with its params object (its worker thread
                                                                             // takes the context's lock: joined before we take it)
  {
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    (void)hipSetDevice(c->device);
    engine_free(p->eng);
    delete p;
  }
  ctx_release(c);
}


// every entry point runs under its context's lock AND on its context's device (hipSetDevice is per thread and cheap): a process that holds
// contexts on several GPUs may call any function of any of them from any thread
#define EG_LOCK(c) std::unique_lock<std::recursive_mutex> lk_; if (c) { lk_ = std::unique_lock<std::recursive_mutex>((c)->mu); (void)hipSetDevice((c)->device); }
#define EG_LOCK_P(p) EG_LOCK((p) ? (p)->eng->ctx : (eg_ctx*)nullptr)

extern "C" {

const char* eg_last_error(void) { return g_err.c_str(); }
int eg_abi_version(void) { return EG_ABI_VERSION; }

int eg_init(int device, eg_ctx** out) {
  if (!out) return fail(EG_ERR_BAD_ARG, "out is null");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(EG_ERR_NO_DEVICE, "no HIP device visible");
  if (device < 0 || device >= count) return fail(EG_ERR_BAD_ARG, "device index out of range");
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  std::unique_ptr<eg_ctx> c(new eg_ctx());
  c->device = device;
  c->cus = prop.multiProcessorCount;
  c->name = std::string(prop.name) + " (" + prop.gcnArchName + ")";
  c->knobs = read_knobs();
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos && !c->knobs.allow_any_arch)
    return fail(EG_ERR_NO_DEVICE, "device is " + c->name + ", this library is built for gfx950 (MI355X) only");
  HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  HIPCHK(hipMalloc((void**)&c->gen_words, 2 * PT_WORDS * sizeof(u32)));
  hipLaunchKernelGGL(k_setup_points, dim3(1), dim3(64), 0, c->stream, (const u32*)nullptr, c->gen_words, (u32*)nullptr);
  {
    const int rc = comb_table_build(c->gen_words, EG_COMB_BITS, c->stream, &c->tabG);
    if (rc) return rc;
  }
  if (c->knobs.comb_big_bits >= 0) c->big_bits = c->knobs.comb_big_bits;
  if (c->knobs.comb_big_min >= 0) c->big_min = (size_t)c->knobs.comb_big_min;
  if (c->big_bits != 0 && (c->big_bits <= EG_COMB_BITS || c->big_bits > 26)) return fail(EG_ERR_BAD_ARG, "EG_COMB_BIG_BITS must be 0 or in (EG_COMB_BITS, 26]");
  int per_cu = 0;
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_eq_table<false, 6>, NT, 0));
  // the shared-chain kernel keeps up to EG_MULTI_GROUP sign vectors per lane in dynamic LDS (9 KiB per term and block)
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_eq_table<true, 5>), hipFuncAttributeMaxDynamicSharedMemorySize,
                             EG_MULTI_GROUP * 9 * NT * (int)sizeof(u32)));
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_eq_table<true, 6>), hipFuncAttributeMaxDynamicSharedMemorySize,
                             EG_MULTI_GROUP * 9 * NT * (int)sizeof(u32)));
#ifdef EG_TEETH7
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_eq_table<true, 7>), hipFuncAttributeMaxDynamicSharedMemorySize,
                             EG_MULTI_GROUP * 9 * NT * (int)sizeof(u32)));
#endif
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_prim_msm<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                             MSM_CHUNK * 8 * NT * (int)sizeof(u32)));
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_prim_msm<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                             MSM_CHUNK * 8 * NT * (int)sizeof(u32)));
  if (per_cu < 1) per_cu = 1;
  c->resident_blocks = per_cu * c->cus;
  // A grid of exactly the resident blocks makes every block do the same number of rounds, so the slowest CU sets the time and the
  // last round runs part-empty; 32 blocks per CU, handed out as others finish, measured +1.5 % (single) / +1.8 % (QV) in one
  // call in round 2 (2 -> 4 -> 8 -> 16 -> 32 -> 64 blocks per CU: 5.33 / 5.38 / 5.41 / 5.39 / 5.40 / 5.44 M ballots/s).  The price is the
  // per-lane workspace: 2.4 GB.
  per_cu = c->knobs.msm_blocks_per_cu;      // 32
  c->msm_blocks = per_cu * c->cus;
  HIPCHK(hipMalloc((void**)&c->ws, (size_t)c->msm_blocks * WS_QUADS * NT * sizeof(uint4)));
  for (hipEvent_t& ev : c->ws_done) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipGetLastError());
  *out = c.release();
  return EG_OK;
}

void eg_destroy(eg_ctx* c) { ctx_release(c); }

int eg_device_name(eg_ctx* c, char* buf, size_t cap) { EG_LOCK(c);
  if (!c || !buf || !cap) return fail(EG_ERR_BAD_ARG, "bad argument");
  snprintf(buf, cap, "%s, %d CUs, msm grid %d blocks", c->name.c_str(), c->cus, c->msm_blocks);
  return EG_OK;
}

int eg_synchronize(eg_ctx* c) { EG_LOCK(c);
  if (!c) return fail(EG_ERR_BAD_ARG, "ctx is null");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipDeviceSynchronize());      // _device / _async work may sit on caller streams, not only on the context's own
  return EG_OK;
}

int eg_profile_enable(eg_ctx* c, int enable) { EG_LOCK(c);
  if (!c) return fail(EG_ERR_BAD_ARG, "ctx is null");
  c->prof = enable != 0;
  c->prof_serial = enable == 2;
  return EG_OK;
}

int eg_profile_read(eg_ctx* c, double* msm_ms_total, uint64_t* msm_launches, double* all_ms_total) { EG_LOCK(c);
  if (!c) return fail(EG_ERR_BAD_ARG, "ctx is null");
  HIPCHK(hipDeviceSynchronize());
  for (auto& sp : c->spans) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, sp.a, sp.b));
    if (sp.kind == PROF_MSM) { c->msm_ms += ms; c->msm_launches++; }
    else if (sp.kind == PROF_TABLES) { c->tables_ms += ms; c->tables_launches++; }
    else c->all_ms += ms;
    c->event_pool.push_back(sp.a);
    c->event_pool.push_back(sp.b);
  }
  c->spans.clear();
  if (msm_ms_total) *msm_ms_total = c->msm_ms;
  if (msm_launches) *msm_launches = c->msm_launches;
  if (all_ms_total) *all_ms_total = c->all_ms;
  c->msm_ms = 0; c->all_ms = 0; c->msm_launches = 0;
  return EG_OK;
}
int eg_profile_read_tables(eg_ctx* c, double* tables_ms_total, uint64_t* tables_launches) { EG_LOCK(c);
  if (!c) return fail(EG_ERR_BAD_ARG, "ctx is null");
  if (tables_ms_total) *tables_ms_total = c->tables_ms;
  if (tables_launches) *tables_launches = c->tables_launches;
  c->tables_ms = 0; c->tables_launches = 0;
  return EG_OK;
}

int eg_selfcheck_generator_table(eg_ctx* c, int wide, size_t samples, uint64_t seed, uint64_t* mismatches) { EG_LOCK(c);
  if (!c || !mismatches) return fail(EG_ERR_BAD_ARG, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  if (wide && !c->tabG_big) {
    if (c->big_bits == 0) return fail(EG_ERR_BAD_ARG, "wide comb tables are switched off (EG_COMB_BIG_BITS=0)");
    const int rc = comb_table_build(c->gen_words, c->big_bits, s, &c->tabG_big, true);
    if (rc == EG_ERR_NOMEM) return fail(EG_ERR_NOMEM, "the wide comb table does not fit the device memory");
    if (rc) return rc;
  }
  unsigned long long* d_bad = nullptr;
  HIPCHK(hipMalloc((void**)&d_bad, sizeof(unsigned long long)));
  HIPCHK(hipMemsetAsync(d_bad, 0, sizeof(unsigned long long), s));
  if (samples)
    hipLaunchKernelGGL(k_check_fixed_table, dim3(blocks_of(samples)), dim3(NT), 0, s, c->gen_words, wide ? c->tabG_big : c->tabG, samples,
                       (u64)seed, d_bad);
  unsigned long long bad = 0;
  const hipError_t he = hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, s);
  const hipError_t se = hipStreamSynchronize(s);
  (void)hipFree(d_bad);
  HIPCHK(he); HIPCHK(se);
  *mismatches = (uint64_t)bad;
  return EG_OK;
}

int eg_comb_table_bits(eg_ctx* c, int* narrow_bits, int* wide_bits) { EG_LOCK(c);
  if (!c) return fail(EG_ERR_BAD_ARG, "ctx is null");
  if (narrow_bits) *narrow_bits = EG_COMB_BITS;
  if (wide_bits) *wide_bits = c->tabG_big ? c->big_bits : 0;
  return EG_OK;
}

// ---- primitive tier ---------------------------------------------------------------------------------------------
struct DevBuf {      // a device buffer owned for the length of one call (batch-tier helpers)
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  int alloc(size_t bytes) { HIPCHK(hipMalloc(&p, std::max<size_t>(bytes, 16))); return EG_OK; }
  int put(const void* src, size_t bytes, hipStream_t s) { if (bytes) HIPCHK(hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, s)); return EG_OK; }
  int get(void* dst, size_t bytes, hipStream_t s) { if (bytes) HIPCHK(hipMemcpyAsync(dst, p, bytes, hipMemcpyDeviceToHost, s)); return EG_OK; }
};
#define TRY(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)
// Host staging of the stateless passes' "host arrays in, host arrays out" entries: device buffers and a stream of the call's own, released
// on every path.  DevBuf above and prim_bufs below stay apart: they work on the context's stream under its lock, and an allocation that
// does not fit is EG_ERR_HIP there and EG_ERR_NOMEM here, so one helper for both would change an error code.
struct HostStage {
  const char* who;                                            // the entry's family: the prefix of its error texts
  std::vector<void*> bufs;
  hipStream_t s = nullptr;
  explicit HostStage(const char* who_) : who(who_) {}
  ~HostStage() {
    for (void* p : bufs) if (p) (void)hipFree(p);
    if (s) (void)hipStreamDestroy(s);
  }
  int open() { HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); return EG_OK; }
  int put(void** out, const void* src, size_t bytes) {        // src null: room only
    void* p = nullptr;
    const hipError_t he = hipMalloc(&p, std::max<size_t>(bytes, 16));
    if (he == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(EG_ERR_NOMEM, std::string(who) + ": the staging buffers do not fit the device memory"); }
    HIPCHK(he);
    bufs.push_back(p);
    if (src && bytes) HIPCHK(hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, s));
    *out = p;
    return EG_OK;
  }
  int get(void* dst, const void* src, size_t bytes) { HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s)); return EG_OK; }
  int sync() { HIPCHK(hipStreamSynchronize(s)); return EG_OK; }
};
// the argument rules of the stateless passes need no context (so they can be tested without a GPU); what passes them fails on a null one
static int check_ctx(const char* who, const eg_ctx* c) { return c ? EG_OK : fail(EG_ERR_BAD_ARG, std::string(who) + ": null ctx"); }
// device pointers of 64-bit and of 32-bit words, or-ed together; a family's two messages name its arguments of either kind
struct AlignedMsgs { const char* words64; const char* words32; };
static int check_aligned(const AlignedMsgs& msgs, uintptr_t words64, uintptr_t words32) {
  if (words64 & 7u) return fail(EG_ERR_BAD_ARG, msgs.words64);
  if (words32 & 3u) return fail(EG_ERR_BAD_ARG, msgs.words32);
  return EG_OK;
}
// The primitive tier works out of ONE device scratch area per context, kept between calls (round 2 paid three to five hipMalloc /
// hipFree per call).  Every primitive call runs under the context lock and ends with a stream synchronisation, so the area is free
// again when the next call starts; it only ever grows.
static int prim_bufs(eg_ctx* c, std::initializer_list<size_t> sizes, std::initializer_list<void**> ptrs) {
  size_t total = 0;
  for (size_t b : sizes) total += (b + 255) / 256 * 256;
  if (total > c->prim_scratch_bytes) {
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->prim_scratch) (void)hipFree(c->prim_scratch);
    c->prim_scratch = nullptr; c->prim_scratch_bytes = 0;
    const size_t want = std::max<size_t>(total + total / 4, (size_t)1 << 20);
    HIPCHK(hipMalloc(&c->prim_scratch, want));
    c->prim_scratch_bytes = want;
  }
  size_t off = 0;
  auto it = ptrs.begin();
  for (size_t b : sizes) { **it = static_cast<char*>(c->prim_scratch) + off; off += (b + 255) / 256 * 256; ++it; }
  return EG_OK;
}
static int h2d(void* dst, const void* src, size_t bytes, hipStream_t s) { if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s)); return EG_OK; }
static int d2h(void* dst, const void* src, size_t bytes, hipStream_t s) { if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s)); return EG_OK; }

int eg_scalar_from_wide_batch(eg_ctx* c, size_t n, const uint8_t* wide, uint8_t* out) { EG_LOCK(c);
  if (!c || (n && (!wide || !out))) return fail(EG_ERR_BAD_ARG, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  void *a, *o;
  TRY(prim_bufs(c, {n * 64, n * 32}, {&a, &o})); TRY(h2d(a, wide, n * 64, c->stream));
  hipLaunchKernelGGL(k_prim_scalar_from_wide, dim3(blocks_of(n)), dim3(NT), 0, c->stream, n, (const u32*)a, (u32*)o);
  TRY(d2h(out, o, n * 32, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return EG_OK;
}
int eg_scalar_is_canonical_batch(eg_ctx* c, size_t n, const uint8_t* s_, uint8_t* ok) { EG_LOCK(c);
  if (!c || (n && (!s_ || !ok))) return fail(EG_ERR_BAD_ARG, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  void *a, *o;
  TRY(prim_bufs(c, {n * 32, n}, {&a, &o})); TRY(h2d(a, s_, n * 32, c->stream));
  hipLaunchKernelGGL(k_prim_scalar_canonical, dim3(blocks_of(n)), dim3(NT), 0, c->stream, n, (const u32*)a, (unsigned char*)o);
  TRY(d2h(ok, o, n, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return EG_OK;
}
int eg_scalar_muladd_batch(eg_ctx* c, size_t n, const uint8_t* a_, const uint8_t* b_, const uint8_t* c_, uint8_t* out) { EG_LOCK(c);
  if (!c || (n && (!a_ || !b_ || !c_ || !out))) return fail(EG_ERR_BAD_ARG, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  void *a, *b, *cc, *o;
  TRY(prim_bufs(c, {n * 32, n * 32, n * 32, n * 32}, {&a, &b, &cc, &o}));
  TRY(h2d(a, a_, n * 32, c->stream)); TRY(h2d(b, b_, n * 32, c->stream)); TRY(h2d(cc, c_, n * 32, c->stream));
  hipLaunchKernelGGL(k_prim_scalar_muladd, dim3(blocks_of(n)), dim3(NT), 0, c->stream, n, (const u32*)a, (const u32*)b,
                     (const u32*)cc, (u32*)o);
  TRY(d2h(out, o, n * 32, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return EG_OK;
}
int eg_scalar_neg_batch(eg_ctx* c, size_t n, const uint8_t* a_, uint8_t* out) { EG_LOCK(c);
  if (!c || (n && (!a_ || !out))) return fail(EG_ERR_BAD_ARG, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  void *a, *o;
  TRY(prim_bufs(c, {n * 32, n * 32}, {&a, &o})); TRY(h2d(a, a_, n * 32, c->stream));
  hipLaunchKernelGGL(k_prim_scalar_neg, dim3(blocks_of(n)), dim3(NT), 0, c->stream, n, (const u32*)a, (u32*)o);
  TRY(d2h(out, o, n * 32, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return EG_OK;
}
int eg_scalar_invert_batch(eg_ctx* c, size_t n, const uint8_t* a_, uint8_t* out) { EG_LOCK(c);
  if (!c || (n && (!a_ || !out))) return fail(EG_ERR_BAD_ARG, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  void *a, *o;
  TRY(prim_bufs(c, {n * 32, n * 32}, {&a, &o})); TRY(h2d(a, a_, n * 32, c->stream));
  hipLaunchKernelGGL(k_prim_scalar_invert, dim3(blocks_of(n)), dim3(NT), 0, c->stream, n, (const u32*)a, (u32*)o);
  TRY(d2h(out, o, n * 32, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return EG_OK;
}
int eg_point_is_identity_batch(eg_ctx* c, size_t n, const uint8_t* in, uint8_t* is_identity, uint8_t* ok) { EG_LOCK(c);
  if (!c || (n && (!in || !is_identity || !ok))) return fail(EG_ERR_BAD_ARG, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  void *a, *f, *o;
  TRY(prim_bufs(c, {n * 32, n, n}, {&a, &f, &o})); TRY(h2d(a, in, n * 32, c->stream));
  hipLaunchKernelGGL(k_prim_point_is_identity, dim3(blocks_of(n)), dim3(NT), 0, c->stream, n, (const u32*)a,
                     (unsigned char*)f, (unsigned char*)o);
  TRY(d2h(is_identity, f, n, c->stream)); TRY(d2h(ok, o, n, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return EG_OK;
}
int eg_point_roundtrip_batch(eg_ctx* c, size_t n, const uint8_t* in, uint8_t* out, uint8_t* ok) { EG_LOCK(c);
  if (!c || (n && (!in || !out || !ok))) return fail(EG_ERR_BAD_ARG, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  void *a, *o, *k;
  TRY(prim_bufs(c, {n * 32, n * 32, n}, {&a, &o, &k})); TRY(h2d(a, in, n * 32, c->stream));
  hipLaunchKernelGGL(k_prim_point_roundtrip, dim3(blocks_of(n)), dim3(NT), 0, c->stream, n, (const u32*)a, (u32*)o,
                     (unsigned char*)k);
  TRY(d2h(out, o, n * 32, c->stream)); TRY(d2h(ok, k, n, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return EG_OK;
}
int eg_point_add_batch(eg_ctx* c, size_t n, const uint8_t* a_, const uint8_t* b_, int subtract, uint8_t* out, uint8_t* ok) { EG_LOCK(c);
  if (!c || (n && (!a_ || !b_ || !out || !ok))) return fail(EG_ERR_BAD_ARG, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  void *a, *b, *o, *k;
  TRY(prim_bufs(c, {n * 32, n * 32, n * 32, n}, {&a, &b, &o, &k}));
  TRY(h2d(a, a_, n * 32, c->stream)); TRY(h2d(b, b_, n * 32, c->stream));
  hipLaunchKernelGGL(k_prim_point_add, dim3(blocks_of(n)), dim3(NT), 0, c->stream, n, (const u32*)a, (const u32*)b, subtract,
                     (u32*)o, (unsigned char*)k);
  TRY(d2h(out, o, n * 32, c->stream)); TRY(d2h(ok, k, n, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return EG_OK;
}
// How the terms of a problem are cut: chunks of up to MSM_CHUNK terms share a doubling chain (less work per term), but a call with few
// terms in all should still cover the chip (a lone 2^16-term product in chunks of 8 keeps only 8192 lanes busy: 3.1 ms; in chunks of 1
// it is 65 536 independent ladders, ~1 ms): the chunk shrinks until the call has ~2 waves per SIMD worth of lanes.
static void msm_plan(const eg_ctx* ctx, size_t n, size_t terms, int* chunk, int* n_chunks) {
  const size_t lanes_wanted = ctx->knobs.msm_lanes;     // 2^17 (EG_MSM_LANES; tests: 1 = always full chunks)
  size_t c = std::min<size_t>(std::max<size_t>(terms, 1), MSM_CHUNK);
  c = std::min(c, std::max<size_t>(1, n * terms / lanes_wanted));
  *chunk = (int)c;
  *n_chunks = (int)std::max<size_t>(1, (terms + c - 1) / c);
}
// scratch of a call that is cut into several chunks per problem: two areas (the folds ping-pong between them), each holding the partial
// sums (PT_WORDS words) and the decode flags (one byte) of up to `count` chunks
struct MsmScratch { u32* part[2]; unsigned char* ok[2]; };
static size_t msm_area_bytes(size_t count) { return (count * PT_WORDS * sizeof(u32) + 255) / 256 * 256 + (count + 255) / 256 * 256; }
static size_t msm_scratch_total(size_t n, size_t nc) { return nc > 1 ? msm_area_bytes(n * nc) + msm_area_bytes(n * ((nc + 63) / 64)) : 0; }
static MsmScratch msm_scratch_at(void* base, size_t n, size_t nc) {
  MsmScratch m{{nullptr, nullptr}, {nullptr, nullptr}};
  if (nc <= 1 || !base) return m;
  char* p = static_cast<char*>(base);
  const size_t c0 = n * nc, c1 = n * ((nc + 63) / 64);
  m.part[0] = reinterpret_cast<u32*>(p); m.ok[0] = reinterpret_cast<unsigned char*>(p + (c0 * PT_WORDS * sizeof(u32) + 255) / 256 * 256);
  p += msm_area_bytes(c0);
  m.part[1] = reinterpret_cast<u32*>(p); m.ok[1] = reinterpret_cast<unsigned char*>(p + (c1 * PT_WORDS * sizeof(u32) + 255) / 256 * 256);
  return m;
}
// `count` partial sums per problem in m.part[0] -> out: 64-fold wavefront-shuffle passes, then one wavefront per problem adds them up, adds the
// generator term and encodes
static void msm_fold_reduce(eg_ctx* c, size_t n, int count, const MsmScratch& m, const u32* d_r, u32* d_out, unsigned char* d_ok, hipStream_t s) {
  int cur = 0;
  while (count > 64) {                 // 64-fold per pass, one wavefront per 64 partial sums
    const int next = (count + 63) / 64;
    hipLaunchKernelGGL(k_prim_msm_fold, dim3((unsigned)((n * (size_t)next * 64 + NT - 1) / NT)), dim3(NT), 0, s, n, count, next,
                       m.part[cur], m.ok[cur], m.part[cur ^ 1], m.ok[cur ^ 1]);
    cur ^= 1; count = next;
  }
  hipLaunchKernelGGL(k_prim_msm_reduce, dim3((unsigned)((n * 64 + NT - 1) / NT)), dim3(NT), 0, s, n, count, m.part[cur], m.ok[cur],
                     d_r, c->tabG, d_out, d_ok);
}

// ---- the bucket method for one very large product (pippenger.cuh) ----------------------------------------------------------------------------
// Window width by size: 2^(c-1) buckets per window with ~64 terms each.  Measured against the Straus path (tools/msm_probe.py,
// profiles/r04_msm_by_size.txt): 2^19 terms 3.6 ms against 3.3, 2^20 4.8 against 5.7, 2^21 7.3 against 10.8, 2^22 13.0 against 21.5 - the
// bucket method takes over from 2^20 terms; EG_MSM_BUCKET_MIN moves the switch (tests force either path at sizes the oracle can follow).
static int pip_window_bits(size_t terms) {
  int c = PIP_MIN_C;
  while (c < PIP_MAX_C && ((size_t)64 << (c - 1)) < terms) ++c;      // 2^17 -> 12, 2^18 -> 13, 2^19 -> 14, >= 2^20 -> 15
  return c;
}
static bool msm_uses_buckets(const eg_ctx* ctx, size_t terms) { return terms >= std::max<size_t>(ctx->knobs.msm_bucket_min, (size_t)1 << 12); }
constexpr int PIP_MAX_LEVELS = PIP_SEQ - 1;
struct PipLayout {
  size_t niels, digits, counts, offsets, cursors, idx, pieces[PIP_MAX_LEVELS], piece0[PIP_MAX_LEVELS], totals, tiles, psum[2], flag, part, total;
  size_t psum_points;       // capacity of each of the two partial-sum buffers
  int c, W, B, waves, levels;
};
static PipLayout pip_layout(size_t terms) {
  PipLayout L;
  L.c = pip_window_bits(terms); L.W = pip_windows(L.c); L.B = 1 << (L.c - 1); L.waves = L.W * (L.B / PIP_SEG) / 64;
  const size_t nb = (size_t)L.W * L.B;
  // levels: pieces of 128 terms, then of 64 partial sums, until the longest possible bucket (all terms) is down to one sum
  L.levels = 1;
  for (size_t n = (terms + PIP_S_TERMS - 1) / PIP_S_TERMS; n > 1; n = (n + PIP_S_POINTS - 1) / PIP_S_POINTS) ++L.levels;
  L.psum_points = (size_t)L.W * terms / PIP_S_TERMS + nb + 64;      // every bucket adds at most one ragged piece per level
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
  L.niels = take(terms * PIP_NIELS_WORDS * sizeof(u32));
  L.digits = take((size_t)L.W * terms * sizeof(unsigned short));
  L.counts = take(nb * sizeof(u32));
  L.offsets = take(nb * sizeof(u32));
  L.cursors = take(nb * sizeof(u32));
  L.idx = take((size_t)L.W * terms * sizeof(u32));
  for (int l = 0; l < PIP_MAX_LEVELS; ++l) { L.pieces[l] = take(nb * sizeof(u32)); L.piece0[l] = take(nb * sizeof(u32)); }
  L.totals = take(256);
  L.tiles = take((size_t)egscan::scan_tiles(nb) * PIP_SEQ * sizeof(u32));
  L.psum[0] = take(L.psum_points * PT_QUADS * sizeof(uint4));
  L.psum[1] = take(L.psum_points * PT_QUADS * sizeof(uint4));
  L.flag = take(256);
  L.part = take(msm_scratch_total(1, (size_t)L.waves) + 256);
  L.total = off;
  return L;
}
static int pip_launch(eg_ctx* c, size_t terms, const u32* d_scalars, const u32* d_points, const u32* d_r, void* d_scratch, u32* d_out,
                      unsigned char* d_ok, hipStream_t s, bool prepared = false) {
  const PipLayout L = pip_layout(terms);
  if (L.levels > PIP_MAX_LEVELS) return fail(EG_ERR_BAD_ARG, "too many terms for the bucket method");
  char* base = static_cast<char*>(d_scratch);
  auto at = [&](size_t o) { return reinterpret_cast<u32*>(base + o); };
  PipBufs P;
  P.niels = at(L.niels); P.digits = reinterpret_cast<unsigned short*>(base + L.digits);
  P.counts = at(L.counts); P.offsets = at(L.offsets); P.cursors = at(L.cursors); P.idx = at(L.idx); P.all_ok = at(L.flag);
  const u32 nb = (u32)((size_t)L.W * L.B);
  u32* totals = at(L.totals);
  uint4* psum[2] = {reinterpret_cast<uint4*>(base + L.psum[0]), reinterpret_cast<uint4*>(base + L.psum[1])};
  HIPCHK(hipMemsetAsync(P.counts, 0, (size_t)nb * sizeof(u32), s));
  HIPCHK(hipMemsetAsync(P.all_ok, 0x01, sizeof(u32), s));
  if (prepared) hipLaunchKernelGGL(k_pip_prepare<true>, dim3((unsigned)((terms + NT - 1) / NT)), dim3(NT), 0, s, terms, L.c, d_scalars, d_points, P);
  else hipLaunchKernelGGL(k_pip_prepare<false>, dim3((unsigned)((terms + NT - 1) / NT)), dim3(NT), 0, s, terms, L.c, d_scalars, d_points, P);
  {
    PipScan S;
    S.offsets = P.offsets; S.cursors = P.cursors; S.totals = totals; S.tile_sums = at(L.tiles);
    for (int l = 0; l < PIP_SEQ - 1; ++l) { S.pieces[l] = at(L.pieces[l]); S.piece0[l] = at(L.piece0[l]); }
    const unsigned tiles = egscan::scan_tiles(nb);
    hipLaunchKernelGGL(k_pip_scan_tiles, dim3(tiles), dim3(NT), 0, s, (const u32*)P.counts, nb, L.levels, S);
    hipLaunchKernelGGL(k_pip_scan_tops, dim3(1), dim3(64 * PIP_SEQ), 0, s, tiles, S);
    hipLaunchKernelGGL(k_pip_scan_apply, dim3(tiles), dim3(NT), 0, s, (const u32*)P.counts, nb, L.levels, S);
  }
  hipLaunchKernelGGL(k_pip_fill, dim3(grid_for(terms * (size_t)L.W, c->cus * 64)), dim3(NT), 0, s, terms, L.c, P);
  // level 0: pieces of the term lists; levels 1 ..: pieces of the partial sums of the level before
  const u32* cnt = P.counts;
  const u32* off = P.offsets;
  size_t bound = L.psum_points;
  for (int l = 0; l < L.levels; ++l) {
    u32 *pieces = at(L.pieces[l]), *piece0 = at(L.piece0[l]);
    const PipLevel lv{cnt, off, pieces, piece0, totals + l};
    const int grid = grid_for(bound, c->cus * 64);
    if (l == 0) hipLaunchKernelGGL(k_pip_sum_terms, dim3(grid), dim3(NT), 0, s, P, lv, nb, psum[0]);
    else hipLaunchKernelGGL(k_pip_sum_points, dim3(grid), dim3(NT), 0, s, (const uint4*)psum[(l - 1) & 1], lv, nb, psum[l & 1]);
    cnt = pieces; off = piece0;
    bound = bound / PIP_S_POINTS + nb + 64;
  }
  const MsmScratch m = msm_scratch_at(base + L.part, 1, (size_t)L.waves);
  hipLaunchKernelGGL(k_pip_window, dim3((unsigned)(((size_t)L.waves * 64 + NT - 1) / NT)), dim3(NT), 0, s, L.c, P,
                     (const uint4*)psum[(L.levels - 1) & 1], cnt, off, m.part[0], m.ok[0]);
  msm_fold_reduce(c, 1, L.waves, m, d_r, d_out, d_ok, s);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

static size_t msm_chunks(const eg_ctx* ctx, size_t n, size_t terms) { int c, k; msm_plan(ctx, n, terms, &c, &k); return (size_t)k; }
// scratch a call needs on the device (0: none)
static size_t msm_scratch_for(const eg_ctx* ctx, size_t n, size_t terms) {
  return msm_uses_buckets(ctx, terms) ? pip_layout(terms).total : msm_scratch_total(n, msm_chunks(ctx, n, terms));
}
// out[i] = enc( sum_t [k_it]P_it + [r_i]G ) on device pointers (kernels.cuh: k_prim_msm, k_prim_msm_fold, k_prim_msm_reduce; very large
// products: pippenger.cuh, one problem after the other); asynchronous on s
static int prim_msm_launch(eg_ctx* c, size_t n, size_t terms, const u32* d_scalars, const u32* d_points, const u32* d_r, void* d_scratch,
                           u32* d_out, unsigned char* d_ok, hipStream_t s, bool prepared = false) {
  const size_t pw = prepared ? PREP_WORDS : 8;          // words per point: a prepared point (96 bytes) or an encoding (32)
  if (msm_uses_buckets(c, terms)) {
    for (size_t i = 0; i < n; ++i)
      TRY(pip_launch(c, terms, d_scalars + i * terms * 8, d_points + i * terms * pw, d_r ? d_r + i * 8 : nullptr, d_scratch, d_out + i * 8,
                     d_ok ? d_ok + i : nullptr, s, prepared));
    return EG_OK;
  }
  int chunk, n_chunks;
  msm_plan(c, n, terms, &chunk, &n_chunks);
  const MsmScratch m = msm_scratch_at(d_scratch, n, (size_t)n_chunks);
  // every lane owns `chunk` tables in the per-lane workspace: the grid shrinks accordingly (the workspace is msm_blocks x one table)
  const int grid = grid_for(n * (size_t)n_chunks, std::max(1, c->msm_blocks / chunk));
  TRY(ws_acquire(c, 3u, s));       // the lanes' tables live in the context's per-lane workspace, which engines with work in flight share
  if (prepared) hipLaunchKernelGGL(k_prim_msm<true>, dim3(grid), dim3(NT), (size_t)chunk * 8 * NT * sizeof(u32), s, n, (int)terms, chunk, n_chunks,
                                   d_scalars, d_points, d_r, c->tabG, c->ws, m.part[0], m.ok[0], d_out, d_ok);
  else hipLaunchKernelGGL(k_prim_msm<false>, dim3(grid), dim3(NT), (size_t)chunk * 8 * NT * sizeof(u32), s, n, (int)terms, chunk, n_chunks, d_scalars,
                          d_points, d_r, c->tabG, c->ws, m.part[0], m.ok[0], d_out, d_ok);
  TRY(ws_release(c, 3u, s));
  if (n_chunks > 1) msm_fold_reduce(c, n, n_chunks, m, d_r, d_out, d_ok, s);
  HIPCHK(hipGetLastError());
  return EG_OK;
}
static int prim_msm(eg_ctx* c, size_t n, size_t terms, const uint8_t* scalars, const uint8_t* points, const uint8_t* r,
                    uint8_t* out, uint8_t* ok) {
  HIPCHK(hipSetDevice(c->device));
  if (n == 0) return EG_OK;
  if (terms > ((size_t)1 << 24) || n > ((size_t)1 << 32)) return fail(EG_ERR_BAD_ARG, "at most 2^24 terms per problem");
  const size_t need = msm_scratch_for(c, n, terms);
  void *sc, *pt, *rr, *o, *k, *scratch;
  TRY(prim_bufs(c, {n * terms * 32, n * terms * 32, n * 32, n * 32, n, need}, {&sc, &pt, &rr, &o, &k, &scratch}));
  TRY(h2d(sc, scalars, n * terms * 32, c->stream)); TRY(h2d(pt, points, n * terms * 32, c->stream));
  if (r) TRY(h2d(rr, r, n * 32, c->stream));
  TRY(prim_msm_launch(c, n, terms, (const u32*)sc, (const u32*)pt, r ? (const u32*)rr : (const u32*)nullptr, need ? scratch : nullptr,
                      (u32*)o, (unsigned char*)k, c->stream));
  TRY(d2h(out, o, n * 32, c->stream));
  if (ok) TRY(d2h(ok, k, n, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipGetLastError());
  return EG_OK;
}
int eg_mul_generator_batch(eg_ctx* c, size_t n, const uint8_t* k, uint8_t* out) { EG_LOCK(c);
  if (!c || (n && (!k || !out))) return fail(EG_ERR_BAD_ARG, "bad argument");
  return prim_msm(c, n, 0, nullptr, nullptr, k, out, nullptr);
}
int eg_vartime_double_mul_generator_batch(eg_ctx* c, size_t n, const uint8_t* k, const uint8_t* p, const uint8_t* r, uint8_t* out,
                                          uint8_t* ok) { EG_LOCK(c);
  if (!c || (n && (!k || !p || !r || !out || !ok))) return fail(EG_ERR_BAD_ARG, "bad argument");
  return prim_msm(c, n, 1, k, p, r, out, ok);
}
int eg_vartime_multi_mul_batch(eg_ctx* c, size_t n, size_t terms, const uint8_t* scalars, const uint8_t* points, uint8_t* out,
                               uint8_t* ok) { EG_LOCK(c);
  if (!c || (n && !out) || (n && terms && (!scalars || !points))) return fail(EG_ERR_BAD_ARG, "bad argument");
  return prim_msm(c, n, terms, scalars, points, nullptr, out, ok);
}
// the same on DEVICE buffers, asynchronous on `stream` (a caller that keeps its operands in HBM pays no copies and no synchronisation;
// what bench.py --workload msm times).  d_scratch must hold eg_msm_scratch_bytes_ctx(ctx, n, terms) bytes (0 for <= 8 terms).
size_t eg_msm_scratch_bytes_ctx(eg_ctx* c, size_t n, size_t terms) { return c ? msm_scratch_for(c, n, terms) : 0; }
int eg_vartime_multi_mul_batch_device(eg_ctx* c, size_t n, size_t terms, const void* d_scalars, const void* d_points, const void* d_r,
                                      void* d_scratch, void* d_out, void* d_ok, void* stream) { EG_LOCK(c);
  if (!c || (n && !d_out) || (n && terms && (!d_scalars || !d_points)) || (n && !terms && !d_r)) return fail(EG_ERR_BAD_ARG, "bad argument");
  if (terms > ((size_t)1 << 24)) return fail(EG_ERR_BAD_ARG, "at most 2^24 terms per problem");
  const size_t need = msm_scratch_for(c, n, terms);
  if (n && need && !d_scratch) return fail(EG_ERR_BAD_ARG, "this call is cut into several chunks per problem (or uses the bucket method) and needs d_scratch (eg_msm_scratch_bytes_ctx)");
  if (n == 0) return EG_OK;
  HIPCHK(hipSetDevice(c->device));
  return prim_msm_launch(c, n, terms, (const u32*)d_scalars, (const u32*)d_points, (const u32*)d_r, need ? d_scratch : nullptr, (u32*)d_out,
                         (unsigned char*)d_ok, (hipStream_t)stream);
}

// Prepared points: decode a point set ONCE, multiply over it many times (ristretto.rs:139-145: vartime_multi_mul takes Elements, which in
// the reference ARE decoded points - its callers never pay a decoding per product; eg_vartime_multi_mul_batch_device, which takes
// encodings, does).
size_t eg_prepared_point_size(void) { return PREP_WORDS * sizeof(u32); }
int eg_points_prepare_device(eg_ctx* c, size_t n, const void* d_encodings, void* d_prepared, void* d_ok, void* stream) { EG_LOCK(c);
  if (!c || (n && (!d_encodings || !d_prepared))) return fail(EG_ERR_BAD_ARG, "bad argument");
  if (n && !d_ok) return fail(EG_ERR_BAD_ARG, "d_ok is mandatory: an encoding that does not decode is prepared as the identity, and this is the only place that says so");
  if (reinterpret_cast<uintptr_t>(d_prepared) & 15u) return fail(EG_ERR_BAD_ARG, "d_prepared must be 16-byte aligned");
  if (n == 0) return EG_OK;
  hipLaunchKernelGGL(k_prim_points_prepare, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, n, (const u32*)d_encodings,
                     (u32*)d_prepared, (unsigned char*)d_ok);
  HIPCHK(hipGetLastError());
  return EG_OK;
}
int eg_vartime_multi_mul_prepared_batch_device(eg_ctx* c, size_t n, size_t terms, const void* d_scalars, const void* d_prepared, const void* d_r,
                                               void* d_scratch, void* d_out, void* stream) { EG_LOCK(c);
  if (!c || (n && !d_out) || (n && terms && (!d_scalars || !d_prepared)) || (n && !terms && !d_r)) return fail(EG_ERR_BAD_ARG, "bad argument");
  if (terms > ((size_t)1 << 24)) return fail(EG_ERR_BAD_ARG, "at most 2^24 terms per problem");
  if (reinterpret_cast<uintptr_t>(d_prepared) & 15u) return fail(EG_ERR_BAD_ARG, "d_prepared must be 16-byte aligned");
  const size_t need = msm_scratch_for(c, n, terms);
  if (n && need && !d_scratch) return fail(EG_ERR_BAD_ARG, "this call is cut into several chunks per problem (or uses the bucket method) and needs d_scratch (eg_msm_scratch_bytes_ctx)");
  if (n == 0) return EG_OK;
  return prim_msm_launch(c, n, terms, (const u32*)d_scalars, (const u32*)d_prepared, (const u32*)d_r, need ? d_scratch : nullptr, (u32*)d_out,
                         nullptr, (hipStream_t)stream, true);
}

// The VALU roof of THIS box: the shipped fe_mul in a bare chain (k_selfbench_fmul), launched back to back for `seconds`; the rate and the
// shader clock are taken over the second half, when the power management has settled (a burst of tens of milliseconds runs 10 % faster:
// profiles/r03_ubench_field_sustained.txt).  Boxes of one pool differ by +-3 %, so a fraction of a constant measured elsewhere cannot tell
// a slow box from a regression.
int eg_selfbench_fmul(eg_ctx* c, double seconds, double* fmul_g_per_s, double* sclk_mhz) { EG_LOCK(c);
  if (!c || !fmul_g_per_s || !(seconds > 0) || seconds > 30) return fail(EG_ERR_BAD_ARG, "bad argument (0 < seconds <= 30)");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int waves_per_simd = 3, blocks = c->cus * waves_per_simd, iters = 20000;       // ~30 ms a launch
  const size_t lds = ((size_t)160 * 1024 / waves_per_simd) / 1024 * 1024;
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_selfbench_fmul), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const size_t lanes = (size_t)blocks * NT, waves = lanes / 64;
  void *d_out = nullptr, *d_st = nullptr;
  TRY(prim_bufs(c, {lanes * 16 * sizeof(u32), waves * sizeof(uint2)}, {&d_out, &d_st}));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPCHK(hipEventCreate(&e0));
  ScopeExit ev{[&]() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }};
  HIPCHK(hipEventCreate(&e1));
  const double ops_per_launch = 2.0 * iters * (double)lanes;
  auto burst = [&](int launches, double* g, double* mhz) -> int {
    HIPCHK(hipEventRecord(e0, s));
    for (int l = 0; l < launches; ++l)
      hipLaunchKernelGGL(k_selfbench_fmul, dim3(blocks), dim3(NT), lds, s, (u32*)d_out, (uint2*)d_st, 12345u + (u32)l, iters);
    HIPCHK(hipEventRecord(e1, s));
    HIPCHK(hipEventSynchronize(e1));
    HIPCHK(hipGetLastError());
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<uint2> st(waves);
    HIPCHK(hipMemcpy(st.data(), d_st, waves * sizeof(uint2), hipMemcpyDeviceToHost));
    std::vector<double> f(waves);
    for (size_t i = 0; i < waves; ++i) f[i] = st[i].y ? (double)st[i].x / ((double)st[i].y * 10.0) * 1e3 : 0.0;     // cycles per 10 ns tick -> MHz
    std::sort(f.begin(), f.end());
    *g = ops_per_launch * launches / (ms * 1e6);
    *mhz = f[waves / 2];
    return EG_OK;
  };
  double g = 0, mhz = 0;
  TRY(burst(1, &g, &mhz));                                   // sizes the halves (and warms the clock up)
  const double one_ms = ops_per_launch / (g * 1e6);
  const int half = std::max(1, (int)(seconds * 500.0 / one_ms));
  TRY(burst(half, &g, &mhz));
  TRY(burst(half, &g, &mhz));
  *fmul_g_per_s = g;
  if (sclk_mhz) *sclk_mhz = mhz;
  return EG_OK;
}

// ---- tally stage (examples/voting.rs:122-177) --------------------------------------------------------------------------
// Params::combine_shares (src/sharing/mod.rs:302-325) with lagrange_coefficients (:139-170): the first `threshold` shares are combined
// by Lagrange interpolation in the exponent.  Every scalar operation (products of the index differences, the batched inversion, the
// scaling) and the multi-scalar multiplication run on the GPU primitives; the host only feeds small integers.
int eg_combine_shares(eg_ctx* c, uint64_t shares, uint64_t threshold, size_t n, const uint64_t* indexes, const uint8_t* dh_elements,
                      uint8_t out[32], int* combined) { EG_LOCK(c);
  if (!c || !combined || !out || (n && (!indexes || !dh_elements)) || threshold < 1 || threshold > shares)
    return fail(EG_ERR_BAD_ARG, "bad argument");
  *combined = 0;
  if (n < threshold) return EG_OK;                         // None: the number of shares is insufficient
  const size_t t = (size_t)threshold;                      // .take(self.threshold)
  for (size_t i = 0; i < t; ++i) {
    if (indexes[i] >= shares) return fail(EG_ERR_BAD_ARG, "share index exceeds the number of participants");   // the reference panics
    for (size_t j = 0; j < i; ++j)
      if (indexes[i] == indexes[j]) return fail(EG_ERR_BAD_ARG, "duplicate share index");
  }
  auto u64_scalar = [](uint64_t v, uint8_t* dst) { memset(dst, 0, 32); memcpy(dst, &v, 8); };
  std::vector<uint8_t> prod(32 * (t + 1)), factor(32 * (t + 1)), zero(32 * (t + 1), 0), tmp(32 * (t + 1));
  // lanes 0..t-1: denominators |prod_j d_ij| with d_ii = index_i + 1; lane t: the scale prod_i (index_i + 1)
  for (size_t i = 0; i <= t; ++i) u64_scalar(1, prod.data() + 32 * i);
  std::vector<int> negative(t, 0);
  for (size_t j = 0; j < t; ++j) {
    for (size_t i = 0; i < t; ++i) {
      const uint64_t a = indexes[i], b = indexes[j];
      if (a > b) negative[i] ^= 1;                         // Ordering::Greater => (true, index - other_index)
      u64_scalar(a == b ? a + 1 : (a > b ? a - b : b - a), factor.data() + 32 * i);
    }
    u64_scalar(indexes[j] + 1, factor.data() + 32 * t);
    TRY(eg_scalar_muladd_batch(c, t + 1, prod.data(), factor.data(), zero.data(), tmp.data()));
    prod.swap(tmp);
  }
  for (size_t i = 0; i < t; ++i)
    if (negative[i]) TRY(eg_scalar_neg_batch(c, 1, prod.data() + 32 * i, prod.data() + 32 * i));
  std::vector<uint8_t> inv(32 * t), coeff(32 * t), scale(32 * t);
  TRY(eg_scalar_invert_batch(c, t, prod.data(), inv.data()));                              // G::invert_scalars
  for (size_t i = 0; i < t; ++i) memcpy(scale.data() + 32 * i, prod.data() + 32 * t, 32);
  TRY(eg_scalar_muladd_batch(c, t, inv.data(), scale.data(), zero.data(), coeff.data()));  // [scale](sum [d_i^-1] S_i) = sum [scale d_i^-1] S_i
  uint8_t ok = 0;
  TRY(eg_vartime_multi_mul_batch(c, 1, t, coeff.data(), dh_elements, out, &ok));
  if (!ok) return fail(EG_ERR_BAD_ARG, "a decryption share is not a valid ristretto255 encoding");
  *combined = 1;
  return EG_OK;
}

// ---- shares of many ciphertexts in one pass (share_combine_kernels.cuh; layout and argument rules: share_combine_host.hpp) ---------------
// Params::combine_shares and VerifiableDecryption::decrypt_to_element for a whole vector of ciphertexts: per-precinct tallies are 10^4 ..
// 10^5 of them, and eg_combine_shares opens one per dozen synchronised calls.  Stateless like the grouped tally: no lock, no workspace of
// the context (only its device number is read), scratch from the caller, three launches per slab of ciphertexts on the caller's stream.
static int combine_batch_check(uint64_t shares, uint64_t threshold, size_t m, int k, const uint64_t* indexes) {
  const char* why = egsc::refuse_sizes(shares, threshold, m);
  if (!why) why = egsc::refuse_columns(shares, k, indexes);
  if (why) return fail(EG_ERR_BAD_ARG, std::string("share combine: ") + why);
  return EG_OK;
}
size_t eg_combine_shares_batch_scratch_bytes(uint64_t threshold, size_t m) { return egsc::scratch_bytes(threshold, m); }
int eg_combine_shares_batch_device(eg_ctx* c, uint64_t shares, uint64_t threshold, size_t m, const void* d_ciphertexts, int k,
                                   const uint64_t* indexes, const void* d_items, const void* d_status, void* d_dh, void* d_plain,
                                   void* d_combined, void* d_used, void* d_bad, void* d_scratch, void* stream) {
  TRY_(combine_batch_check(shares, threshold, m, k, indexes));
  if (m && (!d_ciphertexts || (k && !d_items) || !d_combined || !d_bad)) return fail(EG_ERR_BAD_ARG, "share combine: null device pointer");
  if (egsc::scratch_bytes(threshold, m) && !d_scratch)
    return fail(EG_ERR_BAD_ARG, "share combine: null scratch (eg_combine_shares_batch_scratch_bytes says how much)");
  if (((uintptr_t)d_ciphertexts | (uintptr_t)d_items | (uintptr_t)d_status | (uintptr_t)d_dh | (uintptr_t)d_plain | (uintptr_t)d_combined |
       (uintptr_t)d_bad | (uintptr_t)d_scratch) & 15u)
    return fail(EG_ERR_BAD_ARG, "share combine: device buffers must be 16-byte aligned");
  if ((uintptr_t)d_used & 7u) return fail(EG_ERR_BAD_ARG, "share combine: d_used must be 8-byte aligned");
  if (!c) return fail(EG_ERR_BAD_ARG, "share combine: null context");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  u32* bad = static_cast<u32*>(d_bad);
  if (bad) HIPCHK(hipMemsetAsync(bad, 0, 3 * sizeof(u32), s));
  if (m == 0) return EG_OK;
  const egsc::Layout L = egsc::layout(threshold, m);
  char* base = static_cast<char*>(d_scratch);
  u64* masks = reinterpret_cast<u64*>(base + L.mask);
  u32* coef = reinterpret_cast<u32*>(base + L.coef);
  uint4* tables = reinterpret_cast<uint4*>(base + L.tables);
  ScIndexes idx{};
  for (int j = 0; j < k; ++j) idx.v[j] = (unsigned char)indexes[j];
  const ScStatusDev status{static_cast<const u32*>(d_status), m};
  const ScItemsDev items{static_cast<const uint4*>(d_items), m};
  const ScCtDev cts{static_cast<const uint4*>(d_ciphertexts)};
  const u32 t = (u32)threshold;
  for (size_t first = 0; first < m; first += L.lanes) {
    const u32 count = (u32)std::min(L.lanes, m - first);
    const dim3 grid((count + NT - 1) / NT);
    hipLaunchKernelGGL(k_sc_select, grid, dim3(NT), 0, s, (u32)first, count, k, t, status, items, cts, masks, bad);
    if ((uint64_t)k >= threshold) hipLaunchKernelGGL(k_sc_coeffs, grid, dim3(NT), 0, s, count, k, t, idx, (const u64*)masks, coef, L.lanes);
    hipLaunchKernelGGL(k_sc_combine, grid, dim3(NT), 0, s, (u32)first, count, k, t, L.chunk, idx, items, cts, (const u64*)masks, (const u32*)coef,
                       L.lanes, tables, d_dh, d_plain, static_cast<unsigned char*>(d_combined), static_cast<u64*>(d_used), bad);
  }
  HIPCHK(hipGetLastError());
  return EG_OK;
}
// host buffers, staged into device memory of the call's own
int eg_combine_shares_batch(eg_ctx* c, uint64_t shares, uint64_t threshold, size_t m, const uint8_t* ciphertexts, int k, const uint64_t* indexes,
                            const uint8_t* items, const uint32_t* status, uint8_t* dh, uint8_t* plain, uint8_t* combined, uint64_t* used) {
  TRY_(combine_batch_check(shares, threshold, m, k, indexes));
  if (m && (!ciphertexts || (k && !items) || !combined)) return fail(EG_ERR_BAD_ARG, "share combine: null pointer");
  if (!c) return fail(EG_ERR_BAD_ARG, "share combine: null context");
  if (m == 0) return EG_OK;
  HIPCHK(hipSetDevice(c->device));
  HostStage st("share combine"); TRY_(st.open());
  void *dct, *dit, *dst = nullptr, *ddh, *dpl, *dco, *dus, *dbad, *scratch;
  TRY_(st.put(&dct, ciphertexts, m * 64));
  TRY_(st.put(&dit, items, (size_t)k * m * 128));
  if (status) TRY_(st.put(&dst, status, (size_t)k * m * 4));
  TRY_(st.put(&ddh, nullptr, m * 32)); TRY_(st.put(&dpl, nullptr, m * 32)); TRY_(st.put(&dco, nullptr, m)); TRY_(st.put(&dus, nullptr, m * 8));
  TRY_(st.put(&dbad, nullptr, 16)); TRY_(st.put(&scratch, nullptr, egsc::scratch_bytes(threshold, m)));
  TRY_(eg_combine_shares_batch_device(c, shares, threshold, m, dct, k, indexes, dit, dst, ddh, dpl, dco, dus, dbad, scratch, st.s));
  u32 bad[3] = {0, 0, 0};
  if (dh) TRY_(st.get(dh, ddh, m * 32));
  if (plain) TRY_(st.get(plain, dpl, m * 32));
  TRY_(st.get(combined, dco, m));
  if (used) TRY_(st.get(used, dus, m * 8));
  TRY_(st.get(bad, dbad, sizeof bad));
  TRY_(st.sync());
  if (bad[0] || bad[1] || bad[2])
    return fail(EG_ERR_BAD_ARG, "share combine: " + std::to_string(bad[0]) + " accepted share(s) proven for another ciphertext, " +
                                    std::to_string(bad[1]) + " chosen share(s) that do not decode, " + std::to_string(bad[2]) +
                                    " ciphertext(s) whose blinded element does not decode");
  return EG_OK;
}

// DiscreteLogTable (src/encryption.rs:260-298): [v]G (canonical encoding) -> v for the given values; the products come from the GPU,
// the lookups are a host hash map like the reference's HashMap<Vec<u8>, u64>.
struct eg_dlog_table { std::unordered_map<std::string, uint64_t> map; };
int eg_dlog_table_create(eg_ctx* c, size_t n, const uint64_t* values, eg_dlog_table** out) { EG_LOCK(c);
  if (!c || !out || (n && !values)) return fail(EG_ERR_BAD_ARG, "bad argument");
  std::vector<uint64_t> vals;
  for (size_t i = 0; i < n; ++i) if (values[i] != 0) vals.push_back(values[i]);           // .filter(|&value| value != 0)
  std::vector<uint8_t> sc(32 * vals.size(), 0), enc(32 * vals.size());
  for (size_t i = 0; i < vals.size(); ++i) memcpy(sc.data() + 32 * i, &vals[i], 8);
  if (!vals.empty()) TRY(eg_mul_generator_batch(c, vals.size(), sc.data(), enc.data()));
  std::unique_ptr<eg_dlog_table> t(new eg_dlog_table());
  t->map.reserve(vals.size() * 2);
  for (size_t i = 0; i < vals.size(); ++i) t->map.emplace(std::string(reinterpret_cast<const char*>(enc.data()) + 32 * i, 32), vals[i]);
  *out = t.release();
  return EG_OK;
}
void eg_dlog_table_destroy(eg_dlog_table* t) { delete t; }
// values[i] = discrete log of elements[i] if it is in the table (found[i] = 1); the identity (32 zero bytes) is always 0
int eg_dlog_table_get(const eg_dlog_table* t, size_t n, const uint8_t* elements, uint64_t* values, uint8_t* found) {
  if (!t || (n && (!elements || !values || !found))) return fail(EG_ERR_BAD_ARG, "bad argument");
  static const char zero[32] = {0};
  for (size_t i = 0; i < n; ++i) {
    const char* e = reinterpret_cast<const char*>(elements) + 32 * i;
    if (memcmp(e, zero, 32) == 0) { values[i] = 0; found[i] = 1; continue; }
    auto it = t->map.find(std::string(e, 32));
    found[i] = it != t->map.end();
    values[i] = found[i] ? it->second : 0;
  }
  return EG_OK;
}

// ---- bounded discrete logarithms (dlog_kernels.cuh; range arithmetic: dlog_host.hpp) ---------------------------------------------------
// DiscreteLogTable::new(lo..hi).get(e) for ranges that no table holds: a baby table of 2^baby_bits multiples of [4]B in HBM, built once,
// and giant steps over [lo, hi) in launches of at most LAUNCH_LANES lanes.  After every launch the host reads the candidate list and
// confirms each candidate with the existing primitive ([m]G encoded, compared with the element's bytes); it stops once every element is
// answered.  The solver owns its table and scratch - the context's per-lane workspace is not touched - and every call runs on the
// context's stream under the context's lock, ending with a synchronisation like the primitive tier.
struct eg_dlog_solver {
  eg_ctx* ctx = nullptr;
  int baby_bits = 0;
  u32 slot_mask = 0, max_probe = 0, cand_cap = 0;
  unsigned long long *d_slots = nullptr, *d_cand = nullptr;
  u32 *d_consts = nullptr, *d_scratch = nullptr, *d_count = nullptr;   // d_count[0] = candidates of a launch, [1] = insertions past the probe bound
  size_t scratch_lanes = 0;
  void *d_block = nullptr;          // per-call buffers of one block of elements: encodings, prepared points, done flags
  size_t block_cap = 0;
};
static void dlog_solver_free(eg_dlog_solver* s) {
  if (!s) return;
  for (void* p : {(void*)s->d_slots, (void*)s->d_cand, (void*)s->d_consts, (void*)s->d_scratch, (void*)s->d_count, s->d_block}) if (p) (void)hipFree(p);
  delete s;
}
static int dlog_scratch(eg_dlog_solver* s, size_t lanes) {
  lanes = (lanes + NT - 1) / NT * NT;
  if (lanes <= s->scratch_lanes) return EG_OK;
  HIPCHK(hipStreamSynchronize(s->ctx->stream));
  if (s->d_scratch) (void)hipFree(s->d_scratch);
  s->d_scratch = nullptr; s->scratch_lanes = 0;
  HIPCHK(hipMalloc((void**)&s->d_scratch, (size_t)DLOG_RUN * DLOG_RUN_WORDS * lanes * sizeof(u32)));
  s->scratch_lanes = lanes;
  return EG_OK;
}
static void dlog_niels_words(u32 w[DLOG_RUN_WORDS], const ge& p) {
  ge_niels n; ge_to_niels(n, p);
  for (int j = 0; j < EG_NL; ++j) { w[j] = n.ypx.v[j]; w[EG_NL + j] = n.ymx.v[j]; w[2 * EG_NL + j] = n.xy2d.v[j]; }
}
int eg_dlog_solver_create(eg_ctx* c, int baby_bits, eg_dlog_solver** out) { EG_LOCK(c);
  if (!c || !out) return fail(EG_ERR_BAD_ARG, "bad argument");
  *out = nullptr;
  if (baby_bits == 0) baby_bits = egdlog::BABY_BITS_DEFAULT;
  if (baby_bits < egdlog::BABY_BITS_MIN || baby_bits > egdlog::BABY_BITS_MAX) return fail(EG_ERR_BAD_ARG, "baby_bits must be 0 (default) or in 8..28");
  eg_dlog_solver* s = new eg_dlog_solver();
  ScopeExit drop{[&] { if (s) dlog_solver_free(s); }};
  s->ctx = c; s->baby_bits = baby_bits;
  const size_t entries = (size_t)1 << baby_bits, n_slots = 2 * entries;
  s->slot_mask = (u32)(n_slots - 1);
  s->max_probe = (u32)std::min<size_t>(DLOG_MAX_PROBE, n_slots);
  hipStream_t st = c->stream;
  HIPCHK(hipMalloc((void**)&s->d_slots, n_slots * sizeof(unsigned long long)));
  HIPCHK(hipMalloc((void**)&s->d_consts, 2 * DLOG_RUN_WORDS * sizeof(u32)));
  HIPCHK(hipMalloc((void**)&s->d_count, 2 * sizeof(u32)));
  HIPCHK(hipMemsetAsync(s->d_slots, 0, n_slots * sizeof(unsigned long long), st));
  HIPCHK(hipMemsetAsync(s->d_count, 0, 2 * sizeof(u32), st));
  // the two step points, on the host (the device headers compile for both sides): niels([4]B) and niels(-[4 W]B)
  u32 consts[2 * DLOG_RUN_WORDS];
  {
    ge b4, t; ge_generator(t);
    ge_dbl_full(b4, t); ge_dbl_full(t, b4); b4 = t;
    dlog_niels_words(consts, b4);
    ge w = b4;
    for (int i = 0; i < baby_bits; ++i) { ge_dbl_full(t, w); w = t; }
    ge_neg(t, w);
    dlog_niels_words(consts + DLOG_RUN_WORDS, t);
  }
  TRY(h2d(s->d_consts, consts, sizeof(consts), st));
  const size_t runs = entries / DLOG_RUN, per = std::min<size_t>(runs, egdlog::LAUNCH_LANES);
  TRY(dlog_scratch(s, per));
  for (size_t r0 = 0; r0 < runs; r0 += per) {
    const size_t nr = std::min(per, runs - r0);
    hipLaunchKernelGGL(k_dlog_baby, dim3(blocks_of(nr)), dim3(NT), 0, st, (u32)r0, (u32)nr, (u32)entries, c->tabG, s->d_consts, s->d_scratch,
                       s->scratch_lanes, s->d_slots, s->slot_mask, s->max_probe, s->d_count + 1);
  }
  u32 over = 0;
  TRY(d2h(&over, s->d_count + 1, sizeof(u32), st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  if (over) return fail(EG_ERR_HIP, "internal: the baby table needed a probe sequence beyond its bound");
  c->refs.fetch_add(1);   // dropped by eg_dlog_solver_destroy
  *out = s; s = nullptr;
  return EG_OK;
}
void eg_dlog_solver_destroy(eg_dlog_solver* s) {
  if (!s) return;
  eg_ctx* c = s->ctx;
  {
    EG_LOCK(c);
    (void)hipStreamSynchronize(c->stream);
    dlog_solver_free(s);
  }
  ctx_release(c);
}
uint64_t eg_dlog_solver_max_span(const eg_dlog_solver* s, size_t n) { return s ? egdlog::max_span(s->baby_bits, n) : 0; }
size_t eg_dlog_solver_table_bytes(const eg_dlog_solver* s) { return s ? ((size_t)s->slot_mask + 1) * sizeof(unsigned long long) : 0; }
int eg_dlog_solver_solve(eg_dlog_solver* s, size_t n, const uint8_t* elements, uint64_t lo, uint64_t hi, uint64_t* values, uint8_t* found) {
  eg_ctx* c = s ? s->ctx : nullptr;
  EG_LOCK(c);
  if (!s || (n && (!elements || !values || !found))) return fail(EG_ERR_BAD_ARG, "bad argument");
  egdlog::Range R;
  const int rr = egdlog::plan_range(s->baby_bits, n, lo, hi, &R);
  if (rr == egdlog::RANGE_REVERSED) return fail(EG_ERR_BAD_ARG, "lo > hi");
  if (rr == egdlog::RANGE_TOO_WIDE)
    return fail(EG_ERR_BAD_ARG, "hi - lo is wider than eg_dlog_solver_max_span for this many elements: raise baby_bits (or split the range)");
  static const uint8_t zero[32] = {0};
  for (size_t i = 0; i < n; ++i) { values[i] = 0; found[i] = memcmp(elements + 32 * i, zero, 32) == 0; }   // the identity is always 0
  if (!n || !R.steps) return EG_OK;
  hipStream_t st = c->stream;
  const size_t eb = egdlog::block_elems(n);
  if (eb > s->block_cap) {
    HIPCHK(hipStreamSynchronize(st));
    if (s->d_block) (void)hipFree(s->d_block);
    s->d_block = nullptr; s->block_cap = 0;
    HIPCHK(hipMalloc(&s->d_block, eb * (32 + PREP_WORDS * 4 + 1) + 64));
    // candidates of ONE launch: an element has one true hit, the '-' reading of a hit is rare and a 32-bit tag collides once in 2^32
    // probes, so four per element and a margin is far more than a launch produces; beyond it the call FAILS, it never drops a candidate
    if (s->d_cand) (void)hipFree(s->d_cand);
    s->d_cand = nullptr; s->cand_cap = 0;
    const size_t cap = 4 * eb + 4096;
    HIPCHK(hipMalloc((void**)&s->d_cand, cap * 2 * sizeof(unsigned long long)));
    s->cand_cap = (u32)cap;
    s->block_cap = eb;
  }
  u32* d_prep = (u32*)s->d_block;                                           // 96-byte records first: 16-byte aligned
  u32* d_enc = (u32*)((char*)s->d_block + s->block_cap * PREP_WORDS * 4);
  unsigned char* d_done = (unsigned char*)s->d_block + s->block_cap * (PREP_WORDS * 4 + 32);
  std::vector<unsigned char> done;
  std::vector<unsigned long long> cand;
  for (size_t e0 = 0; e0 < n; e0 += eb) {
    const size_t ne = std::min(eb, n - e0);
    TRY(h2d(d_enc, elements + 32 * e0, ne * 32, st));
    hipLaunchKernelGGL(k_prim_points_prepare, dim3(blocks_of(ne)), dim3(NT), 0, st, ne, (const u32*)d_enc, d_prep, d_done);
    done.assign(ne, 0);
    TRY(d2h(done.data(), d_done, ne, st));
    HIPCHK(hipStreamSynchronize(st));
    size_t open = 0;
    for (size_t i = 0; i < ne; ++i) { done[i] = (!done[i] || found[e0 + i]) ? 1 : 0; open += !done[i]; }   // undecodable, or the identity
    TRY(h2d(d_done, done.data(), ne, st));
    const uint64_t per = egdlog::launch_runs(ne);
    for (uint64_t r0 = 0; r0 < R.runs && open; r0 += per) {
      const uint64_t nr = std::min<uint64_t>(per, R.runs - r0);
      const size_t lanes = ne * (size_t)nr;
      TRY(dlog_scratch(s, lanes));
      HIPCHK(hipMemsetAsync(s->d_count, 0, sizeof(u32), st));
      hipLaunchKernelGGL(k_dlog_giant, dim3(blocks_of(lanes)), dim3(NT), 0, st, (u32)e0, (u32)ne, (const u32*)d_prep, (const unsigned char*)d_done,
                         (u64)lo, (u64)R.span, (u64)r0, (u32)nr, (u64)R.steps, s->baby_bits, c->tabG, s->d_consts, s->d_scratch, s->scratch_lanes,
                         (const unsigned long long*)s->d_slots, s->slot_mask, s->max_probe, s->d_count, s->cand_cap, s->d_cand);
      u32 cnt = 0;
      TRY(d2h(&cnt, s->d_count, sizeof(u32), st));
      HIPCHK(hipStreamSynchronize(st));
      if (cnt > s->cand_cap) return fail(EG_ERR_HIP, "internal: more candidates in one launch than the list holds");
      if (!cnt) continue;
      cand.resize(2 * (size_t)cnt);
      TRY(d2h(cand.data(), s->d_cand, cand.size() * sizeof(unsigned long long), st));
      HIPCHK(hipStreamSynchronize(st));
      // confirm: [m]G encoded against the element itself; a false candidate changes nothing and the search goes on
      std::vector<uint8_t> sc(32 * (size_t)cnt, 0), enc(32 * (size_t)cnt);
      for (u32 k = 0; k < cnt; ++k) memcpy(sc.data() + 32 * (size_t)k, &cand[2 * (size_t)k + 1], 8);
      TRY(prim_msm(c, cnt, 0, nullptr, nullptr, sc.data(), enc.data(), nullptr));
      bool changed = false;
      for (u32 k = 0; k < cnt; ++k) {
        const size_t e = (size_t)cand[2 * (size_t)k];
        if (e < e0 || e >= e0 + ne || done[e - e0]) continue;
        if (memcmp(enc.data() + 32 * (size_t)k, elements + 32 * e, 32) != 0) continue;
        values[e] = cand[2 * (size_t)k + 1]; found[e] = 1; done[e - e0] = 1; --open; changed = true;
      }
      if (changed) TRY(h2d(d_done, done.data(), ne, st));
    }
    HIPCHK(hipStreamSynchronize(st));
  }
  HIPCHK(hipGetLastError());
  return EG_OK;
}

// ---- batch tier: choice ---------------------------------------------------------------------------------------------------
// rings per group of the ring-group walk: EG_RING_GROUP overrides the plan's default (0 = every table of a ballot at once)
static int choice_ring_group() { return read_knobs().ring_group; }     // at the creation of a params object (the plan is built before the engine)
size_t eg_choice_ballot_size(int n_options, int single) { return eghost::choice_ballot_size(n_options, single != 0); }

int eg_choice_params_create(eg_ctx* c, const uint8_t pk[32], int n_options, int single, eg_choice_params** out) { EG_LOCK(c);
  if (!c || !pk || !out) return fail(EG_ERR_BAD_ARG, "bad argument");
  if (n_options < 1 || n_options > 4000) return fail(EG_ERR_BAD_ARG, "n_options must be in 1..4000");
  Engine* e = nullptr;
  TRY(engine_create(c, eghost::build_choice_plan(n_options, single != 0, choice_ring_group()), pk, n_options, &e));
  *out = new eg_choice_params{e, n_options, single};
  return EG_OK;
}
void eg_choice_params_destroy(eg_choice_params* p) { params_destroy(p); }
int eg_verify_choice_batch(eg_choice_params* p, size_t n, const uint8_t* ballots, uint32_t* status, uint8_t* tally_out) { EG_LOCK_P(p);
  if (!p || (n && (!ballots || !status))) return fail(EG_ERR_BAD_ARG, "bad argument");
  EG_WAIT_JSON(p->eng);
  return engine_verify_host(p->eng, n, ballots, status, tally_out);
}
int eg_verify_choice_batch_device(eg_choice_params* p, size_t n, const void* d_ballots, void* d_status, void* stream) { EG_LOCK_P(p);
  if (!p || (n && (!d_ballots || !d_status))) return fail(EG_ERR_BAD_ARG, "bad argument");
  EG_WAIT_JSON(p->eng);
  HIPCHK(hipSetDevice(p->eng->ctx->device));
  return engine_verify_device(p->eng, n, d_ballots, d_status, (hipStream_t)stream);
}
static int tally_reset(Engine* e, hipStream_t s, bool wait) {
  if (wait) HIPCHK(hipDeviceSynchronize());   // host form: order after anything still running on caller streams
  hipLaunchKernelGGL(k_tally_init, dim3(blocks_of(e->plan.tally_slots.size())), dim3(NT), 0, s, e->tally, (int)e->plan.tally_slots.size());
  HIPCHK(hipGetLastError());
  TRY(engine_touch(e, s));
  if (wait) HIPCHK(hipStreamSynchronize(s));
  return EG_OK;
}
static int tally_encode_device(Engine* e, void* d_out, hipStream_t s) {
  hipLaunchKernelGGL(k_tally_encode, dim3(blocks_of(e->plan.tally_slots.size())), dim3(NT), 0, s, e->tally, (int)e->plan.tally_slots.size(), (u32*)d_out);
  HIPCHK(hipGetLastError());
  return EG_OK;
}
int eg_choice_tally_encode_device(eg_choice_params* p, void* d_out, void* stream) { EG_LOCK_P(p);
  if (!p || !d_out) return fail(EG_ERR_BAD_ARG, "bad argument");
  EG_WAIT_JSON(p->eng);
  return tally_encode_device(p->eng, d_out, (hipStream_t)stream);
}
int eg_qv_tally_encode_device(eg_qv_params* p, void* d_out, void* stream) { EG_LOCK_P(p);
  if (!p || !d_out) return fail(EG_ERR_BAD_ARG, "bad argument");
  EG_WAIT_JSON(p->eng);
  return tally_encode_device(p->eng, d_out, (hipStream_t)stream);
}
int eg_points_sum_device(eg_ctx* c, int n_ranks, int n_points, const void* d_in, void* d_out, void* d_bad, void* stream) { EG_LOCK(c);
  if (!c || n_ranks < 1 || n_points < 1 || !d_in || !d_out) return fail(EG_ERR_BAD_ARG, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_points_sum, dim3((n_points + 63) / 64), dim3(64), 0, s, (const u32*)d_in, n_ranks, n_points, (u32*)d_out,
                     (u32*)d_bad);
  HIPCHK(hipGetLastError());
  return EG_OK;
}
// ---- per-group tally of a verified batch (group_tally_kernels.cuh) ---------------------------------------------------------------------
// Reads the engine's immutable plan data only (stride, the tally items uploaded at creation): no lock, no workspace, no running tally.
static size_t grouped_scratch_bytes(const Engine* e, size_t n, uint32_t n_groups) {
  if (!e || eggt::refuse(n, n_groups)) return 0;
  return eggt::layout(n, n_groups, (uint32_t)e->plan.tally_slots.size()).total;
}
static int grouped_check(const Engine* e, size_t n, uint32_t n_groups) {
  if (const char* why = eggt::refuse(n, n_groups)) return fail(EG_ERR_BAD_ARG, std::string("grouped tally: ") + why);
  if (!e) return fail(EG_ERR_BAD_ARG, "grouped tally: null params");
  return EG_OK;
}
// the scan of the group counts in the caller's scratch: list offsets, pieces and first piece per group for every level (three launches)
static GtScan grouped_scan(const eggt::Layout& L, char* base, uint32_t n_groups, hipStream_t s) {
  auto at = [&](size_t o) { return reinterpret_cast<u32*>(base + o); };
  GtScan S;
  S.offsets = at(L.offsets); S.totals = at(L.totals); S.tile_sums = at(L.tiles);
  for (int l = 0; l < eggt::MAX_LEVELS; ++l) { S.pieces[l] = at(L.pieces[l]); S.piece0[l] = at(L.piece0[l]); }
  const u32* counts = at(L.counts);
  hipLaunchKernelGGL(k_gt_scan_tiles, dim3(L.n_tiles), dim3(NT), 0, s, counts, n_groups, L.n_levels, eggt::S1, eggt::S2, S);
  hipLaunchKernelGGL(k_gt_scan_tops, dim3(1), dim3(64 * GT_SEQ), 0, s, L.n_tiles, S);
  hipLaunchKernelGGL(k_gt_scan_apply, dim3(L.n_tiles), dim3(NT), 0, s, counts, n_groups, L.n_levels, eggt::S1, eggt::S2, S);
  return S;
}
static int grouped_launch(Engine* e, size_t n, const void* d_ballots, const void* d_status, const void* d_groups, uint32_t n_groups,
                          void* d_scratch, void* d_tallies, void* d_counts, void* d_bad, hipStream_t s) {
  TRY_(grouped_check(e, n, n_groups));
  if (n && (!d_ballots || !d_status || !d_groups || !d_tallies || !d_bad)) return fail(EG_ERR_BAD_ARG, "grouped tally: null device pointer");
  if (!d_tallies) return EG_OK;                                          // n == 0 and nowhere to write the zero tallies to
  const u32 T = (u32)e->plan.tally_slots.size();
  const eggt::Layout L = eggt::layout(n, n_groups, T);
  if (L.total && !d_scratch) return fail(EG_ERR_BAD_ARG, "grouped tally: null scratch (eg_*_tally_grouped_scratch_bytes says how much)");
  if (((uintptr_t)d_ballots | (uintptr_t)d_scratch) & 15u) return fail(EG_ERR_BAD_ARG, "grouped tally: ballots and scratch must be 16-byte aligned");
  if (((uintptr_t)d_status | (uintptr_t)d_groups | (uintptr_t)d_tallies | (uintptr_t)d_counts | (uintptr_t)d_bad) & 3u)
    return fail(EG_ERR_BAD_ARG, "grouped tally: misaligned device pointer");
  if (L.n_levels > eggt::MAX_LEVELS) return fail(EG_ERR_BAD_ARG, "grouped tally: too many ballots");
  HIPCHK(hipSetDevice(e->ctx->device));
  char* base = static_cast<char*>(d_scratch);
  auto at = [&](size_t o) { return reinterpret_cast<u32*>(base + o); };
  u32 *counts = at(L.counts), *cursors = at(L.cursors), *offsets = at(L.offsets), *totals = at(L.totals), *idx = at(L.idx);
  uint4* psum[2] = {reinterpret_cast<uint4*>(base + L.psum[0]), reinterpret_cast<uint4*>(base + L.psum[1])};
  const u32* status = static_cast<const u32*>(d_status);
  const u32* groups = static_cast<const u32*>(d_groups);
  u32* bad = static_cast<u32*>(d_bad);
  const int cap = e->ctx->cus * 64;
  if (bad) HIPCHK(hipMemsetAsync(bad, 0, 2 * sizeof(u32), s));
  HIPCHK(hipMemsetAsync(counts, 0, L.offsets - L.counts, s));          // counts and cursors
  if (n) hipLaunchKernelGGL(k_gt_count, dim3(blocks_of(n)), dim3(NT), 0, s, (u32)n, status, groups, n_groups, counts, bad);
  const GtScan S = grouped_scan(L, static_cast<char*>(d_scratch), n_groups, s);
  const u32 *cnt = counts, *off = offsets;
  if (n) {
    hipLaunchKernelGGL(k_gt_fill, dim3(blocks_of(n)), dim3(NT), 0, s, (u32)n, status, groups, n_groups, (const u32*)offsets, cursors, idx);
    // level 0: pieces of the ballot lists, summed from the wire; levels 1 ..: pieces of the partial sums of the level before
    for (int l = 0; l < L.n_levels; ++l) {
      const GtLevel lv{cnt, off, S.piece0[l]};
      const int grid = grid_for(L.psum_points[l & 1] * T, cap);          // (levels >= 2 have no more pieces than the level two before)
      if (l == 0)
        hipLaunchKernelGGL(k_gt_sum_wire, dim3(grid), dim3(NT), 0, s, eggt::S1, T, lv, (const u32*)(totals + l), n_groups, (const u32*)idx,
                           GtWireDev{static_cast<const u32*>(d_ballots), (u32)(e->plan.stride / 4), (u32)n}, (const u32*)e->d_tally_items, psum[0], bad);
      else
        hipLaunchKernelGGL(k_gt_sum_points, dim3(grid), dim3(NT), 0, s, eggt::S2, T, lv, (const u32*)(totals + l), n_groups,
                           (const uint4*)psum[(l - 1) & 1], psum[l & 1]);
      cnt = S.pieces[l]; off = S.piece0[l];
    }
  }
  const int last = L.n_levels - 1;
  hipLaunchKernelGGL(k_gt_encode, dim3(grid_for((size_t)n_groups * T, cap)), dim3(NT), 0, s, n_groups, T, (const u32*)S.pieces[last],
                     (const u32*)S.piece0[last], (const uint4*)psum[last & 1], (const u32*)counts, static_cast<u32*>(d_tallies),
                     static_cast<u32*>(d_counts));
  HIPCHK(hipGetLastError());
  return EG_OK;
}
// host buffers: stages everything in device memory of its own, runs the pass on a stream of its own and waits for it
static int grouped_host(Engine* e, size_t n, const uint8_t* ballots, const uint32_t* status, const uint32_t* groups, uint32_t n_groups,
                        uint8_t* tallies, uint32_t* counts) {
  TRY_(grouped_check(e, n, n_groups));
  if (!tallies || (n && (!ballots || !status || !groups))) return fail(EG_ERR_BAD_ARG, "grouped tally: null pointer");
  HIPCHK(hipSetDevice(e->ctx->device));
  const size_t T = e->plan.tally_slots.size(), stride = e->plan.stride;
  HostStage st("grouped tally"); TRY_(st.open());
  void *db, *dst, *dg, *scratch, *dt, *dc;
  TRY_(st.put(&db, ballots, n * stride)); TRY_(st.put(&dst, status, n * 4)); TRY_(st.put(&dg, groups, n * 4));
  TRY_(st.put(&scratch, nullptr, grouped_scratch_bytes(e, n, n_groups)));
  TRY_(st.put(&dt, nullptr, (size_t)n_groups * T * 32));
  TRY_(st.put(&dc, nullptr, (size_t)n_groups * 4 + 8));                   // the counts, then the two bad counters
  u32* d_counts = static_cast<u32*>(dc);
  u32* d_bad = d_counts + n_groups;
  TRY_(grouped_launch(e, n, db, dst, dg, n_groups, scratch, dt, d_counts, d_bad, st.s));
  u32 bad[2] = {0, 0};
  TRY_(st.get(tallies, dt, (size_t)n_groups * T * 32));
  if (counts) TRY_(st.get(counts, d_counts, (size_t)n_groups * 4));
  TRY_(st.get(bad, d_bad, sizeof bad));
  TRY_(st.sync());
  if (bad[0] || bad[1])
    return fail(EG_ERR_BAD_ARG, "grouped tally: " + std::to_string(bad[0]) + " accepted ballot(s) with a group id out of range, " +
                                    std::to_string(bad[1]) + " tally point(s) of accepted ballots that do not decode: discard the tallies");
  return EG_OK;
}
size_t eg_choice_tally_grouped_scratch_bytes(const eg_choice_params* p, size_t n, uint32_t n_groups) { return grouped_scratch_bytes(p ? p->eng : nullptr, n, n_groups); }
size_t eg_qv_tally_grouped_scratch_bytes(const eg_qv_params* p, size_t n, uint32_t n_groups) { return grouped_scratch_bytes(p ? p->eng : nullptr, n, n_groups); }
int eg_choice_tally_grouped_device(eg_choice_params* p, size_t n, const void* d_ballots, const void* d_status, const void* d_groups, uint32_t n_groups,
                                   void* d_scratch, void* d_tallies, void* d_counts, void* d_bad, void* stream) {
  return grouped_launch(p ? p->eng : nullptr, n, d_ballots, d_status, d_groups, n_groups, d_scratch, d_tallies, d_counts, d_bad, (hipStream_t)stream);
}
int eg_qv_tally_grouped_device(eg_qv_params* p, size_t n, const void* d_ballots, const void* d_status, const void* d_groups, uint32_t n_groups,
                               void* d_scratch, void* d_tallies, void* d_counts, void* d_bad, void* stream) {
  return grouped_launch(p ? p->eng : nullptr, n, d_ballots, d_status, d_groups, n_groups, d_scratch, d_tallies, d_counts, d_bad, (hipStream_t)stream);
}
int eg_choice_tally_grouped(eg_choice_params* p, size_t n, const uint8_t* ballots, const uint32_t* status, const uint32_t* groups, uint32_t n_groups,
                            uint8_t* tallies, uint32_t* counts) {
  return grouped_host(p ? p->eng : nullptr, n, ballots, status, groups, n_groups, tallies, counts);
}
int eg_qv_tally_grouped(eg_qv_params* p, size_t n, const uint8_t* ballots, const uint32_t* status, const uint32_t* groups, uint32_t n_groups,
                        uint8_t* tallies, uint32_t* counts) {
  return grouped_host(p ? p->eng : nullptr, n, ballots, status, groups, n_groups, tallies, counts);
}
// ---- weighted per-group tally: the same pass with [weight] x point at level 0 and the sums of weights beside the points -----------------
// Stateless like the grouped pass: the plan's immutable data only.
static size_t weighted_scratch_bytes(const Engine* e, size_t n, uint32_t n_groups) {
  if (!e || eggt::refuse(n, n_groups)) return 0;
  return eggt::layout_weighted(n, n_groups, (uint32_t)e->plan.tally_slots.size()).total;
}
static int weighted_check(const Engine* e, size_t n, uint32_t n_groups, int weight_bits, bool have_weights, bool have_groups) {
  const char* why = eggt::refuse(n, n_groups);
  if (!why) why = eggt::refuse_weight_bits(weight_bits);
  if (!why && n && !have_weights) why = "null weights";
  if (!why && !have_groups && n_groups != 1) why = "null groups stand for one group: n_groups must be 1";
  if (why) return fail(EG_ERR_BAD_ARG, std::string("weighted tally: ") + why);
  if (!e) return fail(EG_ERR_BAD_ARG, "weighted tally: null params");
  return EG_OK;
}
static int weighted_launch(Engine* e, size_t n, const void* d_ballots, const void* d_status, const void* d_weights, int weight_bits,
                           const void* d_groups, uint32_t n_groups, void* d_scratch, void* d_tallies, void* d_weight_sums, void* d_counts,
                           void* d_bad, hipStream_t s) {
  TRY_(weighted_check(e, n, n_groups, weight_bits, d_weights != nullptr, d_groups != nullptr));
  if (n && (!d_ballots || !d_status || !d_tallies || !d_bad)) return fail(EG_ERR_BAD_ARG, "weighted tally: null device pointer");
  if (!d_tallies) return EG_OK;                                          // n == 0 and nowhere to write the zero tallies to
  const u32 T = (u32)e->plan.tally_slots.size();
  const eggt::WeightedLayout W = eggt::layout_weighted(n, n_groups, T);
  const eggt::Layout& L = W.base;
  if (W.total && !d_scratch) return fail(EG_ERR_BAD_ARG, "weighted tally: null scratch (eg_*_tally_weighted_scratch_bytes says how much)");
  if (((uintptr_t)d_ballots | (uintptr_t)d_scratch) & 15u) return fail(EG_ERR_BAD_ARG, "weighted tally: ballots and scratch must be 16-byte aligned");
  if (((uintptr_t)d_weights | (uintptr_t)d_weight_sums) & 7u) return fail(EG_ERR_BAD_ARG, "weighted tally: weights and weight sums must be 8-byte aligned");
  if (((uintptr_t)d_status | (uintptr_t)d_groups | (uintptr_t)d_tallies | (uintptr_t)d_counts | (uintptr_t)d_bad) & 3u)
    return fail(EG_ERR_BAD_ARG, "weighted tally: misaligned device pointer");
  if (L.n_levels > eggt::MAX_LEVELS) return fail(EG_ERR_BAD_ARG, "weighted tally: too many ballots");
  HIPCHK(hipSetDevice(e->ctx->device));
  char* base = static_cast<char*>(d_scratch);
  auto at = [&](size_t o) { return reinterpret_cast<u32*>(base + o); };
  u32 *counts = at(L.counts), *cursors = at(L.cursors), *offsets = at(L.offsets), *totals = at(L.totals), *idx = at(L.idx);
  uint4* psum[2] = {reinterpret_cast<uint4*>(base + L.psum[0]), reinterpret_cast<uint4*>(base + L.psum[1])};
  u64* wsum[2] = {reinterpret_cast<u64*>(base + W.wsum[0]), reinterpret_cast<u64*>(base + W.wsum[1])};
  const u32* status = static_cast<const u32*>(d_status);
  const u32* groups = static_cast<const u32*>(d_groups);
  const GtWeightsDev weights{static_cast<const u64*>(d_weights), (u32)n};
  u32* bad = static_cast<u32*>(d_bad);
  const int cap = e->ctx->cus * 64;
  if (bad) HIPCHK(hipMemsetAsync(bad, 0, 3 * sizeof(u32), s));
  HIPCHK(hipMemsetAsync(counts, 0, L.offsets - L.counts, s));          // counts and cursors
  if (n) hipLaunchKernelGGL(k_gtw_count, dim3(blocks_of(n)), dim3(NT), 0, s, (u32)n, status, groups, n_groups, weights, weight_bits, counts, bad);
  const GtScan S = grouped_scan(L, static_cast<char*>(d_scratch), n_groups, s);
  const u32 *cnt = counts, *off = offsets;
  if (n) {
    hipLaunchKernelGGL(k_gtw_fill, dim3(blocks_of(n)), dim3(NT), 0, s, (u32)n, status, groups, n_groups, weights, weight_bits,
                       (const u32*)offsets, cursors, idx);
    for (int l = 0; l < L.n_levels; ++l) {
      const GtLevel lv{cnt, off, S.piece0[l]};
      const size_t cap_pieces = L.psum_points[l & 1];
      const int grid = grid_for(cap_pieces * T, cap);
      if (l == 0) {
        hipLaunchKernelGGL(k_gtw_sum_wire, dim3(grid), dim3(NT), 0, s, eggt::S1, T, lv, (const u32*)(totals + l), n_groups, (const u32*)idx,
                           GtWireDev{static_cast<const u32*>(d_ballots), (u32)(e->plan.stride / 4), (u32)n}, (const u32*)e->d_tally_items,
                           weights, weight_bits, psum[0], wsum[0], bad);
      } else {
        hipLaunchKernelGGL(k_gt_sum_points, dim3(grid), dim3(NT), 0, s, eggt::S2, T, lv, (const u32*)(totals + l), n_groups,
                           (const uint4*)psum[(l - 1) & 1], psum[l & 1]);
        if (d_weight_sums)
          hipLaunchKernelGGL(k_gtw_weight_sums, dim3(grid_for(cap_pieces, cap)), dim3(NT), 0, s, eggt::S2, lv, (const u32*)(totals + l), n_groups,
                             (const u64*)wsum[(l - 1) & 1], wsum[l & 1]);
      }
      cnt = S.pieces[l]; off = S.piece0[l];
    }
  }
  const int last = L.n_levels - 1;
  hipLaunchKernelGGL(k_gt_encode, dim3(grid_for((size_t)n_groups * T, cap)), dim3(NT), 0, s, n_groups, T, (const u32*)S.pieces[last],
                     (const u32*)S.piece0[last], (const uint4*)psum[last & 1], (const u32*)counts, static_cast<u32*>(d_tallies),
                     static_cast<u32*>(d_counts));
  if (d_weight_sums)
    hipLaunchKernelGGL(k_gtw_weight_sums_out, dim3(grid_for(n_groups, cap)), dim3(NT), 0, s, n_groups, (const u32*)S.pieces[last],
                       (const u32*)S.piece0[last], (const u64*)wsum[last & 1], static_cast<u64*>(d_weight_sums));
  HIPCHK(hipGetLastError());
  return EG_OK;
}
// host buffers, staged as grouped_host stages them
static int weighted_host(Engine* e, size_t n, const uint8_t* ballots, const uint32_t* status, const uint64_t* weights, int weight_bits,
                         const uint32_t* groups, uint32_t n_groups, uint8_t* tallies, uint64_t* weight_sums, uint32_t* counts) {
  TRY_(weighted_check(e, n, n_groups, weight_bits, weights != nullptr, groups != nullptr));
  if (!tallies || (n && (!ballots || !status))) return fail(EG_ERR_BAD_ARG, "weighted tally: null pointer");
  HIPCHK(hipSetDevice(e->ctx->device));
  const size_t T = e->plan.tally_slots.size(), stride = e->plan.stride;
  HostStage st("weighted tally"); TRY_(st.open());
  void *db, *dst, *dw, *dg = nullptr, *scratch, *dt, *dsum, *dc;
  TRY_(st.put(&db, ballots, n * stride)); TRY_(st.put(&dst, status, n * 4)); TRY_(st.put(&dw, weights, n * 8));
  if (groups) TRY_(st.put(&dg, groups, n * 4));
  TRY_(st.put(&scratch, nullptr, weighted_scratch_bytes(e, n, n_groups)));
  TRY_(st.put(&dt, nullptr, (size_t)n_groups * T * 32));
  TRY_(st.put(&dsum, nullptr, (size_t)n_groups * 16));
  TRY_(st.put(&dc, nullptr, (size_t)n_groups * 4 + 12));                  // the counts, then the three bad counters
  u32* d_counts = static_cast<u32*>(dc);
  u32* d_bad = d_counts + n_groups;
  TRY_(weighted_launch(e, n, db, dst, dw, weight_bits, dg, n_groups, scratch, dt, dsum, d_counts, d_bad, st.s));
  u32 bad[3] = {0, 0, 0};
  TRY_(st.get(tallies, dt, (size_t)n_groups * T * 32));
  if (weight_sums) TRY_(st.get(weight_sums, dsum, (size_t)n_groups * 16));
  if (counts) TRY_(st.get(counts, d_counts, (size_t)n_groups * 4));
  TRY_(st.get(bad, d_bad, sizeof bad));
  TRY_(st.sync());
  if (bad[0] || bad[1] || bad[2])
    return fail(EG_ERR_BAD_ARG, "weighted tally: " + std::to_string(bad[0]) + " accepted ballot(s) with a group id out of range, " +
                                    std::to_string(bad[1]) + " tally point(s) of accepted ballots that do not decode, " + std::to_string(bad[2]) +
                                    " weight(s) of 2^weight_bits or more: discard the tallies");
  return EG_OK;
}
size_t eg_choice_tally_weighted_scratch_bytes(const eg_choice_params* p, size_t n, uint32_t n_groups) { return weighted_scratch_bytes(p ? p->eng : nullptr, n, n_groups); }
size_t eg_qv_tally_weighted_scratch_bytes(const eg_qv_params* p, size_t n, uint32_t n_groups) { return weighted_scratch_bytes(p ? p->eng : nullptr, n, n_groups); }
int eg_choice_tally_weighted_device(eg_choice_params* p, size_t n, const void* d_ballots, const void* d_status, const void* d_weights, int weight_bits,
                                    const void* d_groups, uint32_t n_groups, void* d_scratch, void* d_tallies, void* d_weight_sums, void* d_counts,
                                    void* d_bad, void* stream) {
  return weighted_launch(p ? p->eng : nullptr, n, d_ballots, d_status, d_weights, weight_bits, d_groups, n_groups, d_scratch, d_tallies,
                         d_weight_sums, d_counts, d_bad, (hipStream_t)stream);
}
int eg_qv_tally_weighted_device(eg_qv_params* p, size_t n, const void* d_ballots, const void* d_status, const void* d_weights, int weight_bits,
                                const void* d_groups, uint32_t n_groups, void* d_scratch, void* d_tallies, void* d_weight_sums, void* d_counts,
                                void* d_bad, void* stream) {
  return weighted_launch(p ? p->eng : nullptr, n, d_ballots, d_status, d_weights, weight_bits, d_groups, n_groups, d_scratch, d_tallies,
                         d_weight_sums, d_counts, d_bad, (hipStream_t)stream);
}
int eg_choice_tally_weighted(eg_choice_params* p, size_t n, const uint8_t* ballots, const uint32_t* status, const uint64_t* weights, int weight_bits,
                             const uint32_t* groups, uint32_t n_groups, uint8_t* tallies, uint64_t* weight_sums, uint32_t* counts) {
  return weighted_host(p ? p->eng : nullptr, n, ballots, status, weights, weight_bits, groups, n_groups, tallies, weight_sums, counts);
}
int eg_qv_tally_weighted(eg_qv_params* p, size_t n, const uint8_t* ballots, const uint32_t* status, const uint64_t* weights, int weight_bits,
                         const uint32_t* groups, uint32_t n_groups, uint8_t* tallies, uint64_t* weight_sums, uint32_t* counts) {
  return weighted_host(p ? p->eng : nullptr, n, ballots, status, weights, weight_bits, groups, n_groups, tallies, weight_sums, counts);
}
// ---- ballot weeding: accepted ballots that repeat a tally ciphertext of the board or of an earlier ballot (weed_kernels.cuh) ----------------
// Stateless like the grouped pass: the plan's immutable data only (stride, tally items, the adjacency checked at creation).
static uint32_t weed_keys_per_ballot(const Engine* e) { return (uint32_t)(e->plan.tally_slots.size() / 2); }
static size_t weed_scratch_bytes(const Engine* e, size_t n, size_t n_prior) {
  if (!e || !e->weed_keys_ok || egw::refuse(n, n_prior, n_prior) || egw::refuse_keys(n, n_prior, weed_keys_per_ballot(e))) return 0;
  return egw::layout(n, n_prior, weed_keys_per_ballot(e)).total;
}
// what both forms refuse before they look at the params object; `append`: the caller asked for the board to be extended
static int weed_check(const Engine* e, size_t n, size_t n_prior, size_t board_cap, bool have_ballots, bool have_dup_of, bool have_found,
                      bool have_board, bool append) {
  const char* why = egw::refuse(n, n_prior, board_cap);
  if (!why && n && !have_ballots) why = "null ballots";
  if (!why && n && !have_dup_of) why = "null dup_of";
  if (!why && n && !have_found) why = "null found";
  if (!why && !have_board && n_prior) why = "null board with n_prior > 0";
  if (!why && !have_board && append) why = "null board with an append requested";
  if (why) return fail(EG_ERR_BAD_ARG, std::string("weed: ") + why);
  if (!e) return fail(EG_ERR_BAD_ARG, "weed: null params");
  if (!e->weed_keys_ok) return fail(EG_ERR_BAD_ARG, "weed: internal: the tally ciphertexts of this plan are not contiguous wire items");
  if ((why = egw::refuse_keys(n, n_prior, weed_keys_per_ballot(e)))) return fail(EG_ERR_BAD_ARG, std::string("weed: ") + why);
  return EG_OK;
}
static int weed_launch(Engine* e, size_t n, const void* d_ballots, const void* d_status, size_t n_prior, void* d_board, size_t board_cap,
                       uint64_t hash_seed, void* d_scratch, void* d_dup_of, void* d_status_out, void* d_board_count, void* d_found, hipStream_t s) {
  if (((uintptr_t)d_ballots | (uintptr_t)d_board | (uintptr_t)d_scratch) & 15u)
    return fail(EG_ERR_BAD_ARG, "weed: ballots, board and scratch must be 16-byte aligned");
  if (((uintptr_t)d_status | (uintptr_t)d_dup_of | (uintptr_t)d_status_out | (uintptr_t)d_found) & 3u || ((uintptr_t)d_board_count & 7u))
    return fail(EG_ERR_BAD_ARG, "weed: misaligned device pointer");
  TRY_(weed_check(e, n, n_prior, board_cap, d_ballots != nullptr, d_dup_of != nullptr, d_found != nullptr, d_board != nullptr,
                  d_board_count != nullptr));
  const u32 K = weed_keys_per_ballot(e);
  const egw::Layout L = egw::layout(n, n_prior, K);
  if (L.total && !d_scratch) return fail(EG_ERR_BAD_ARG, "weed: null scratch (eg_*_weed_scratch_bytes says how much)");
  if (!d_found && !d_board_count) return EG_OK;                          // n == 0 and nowhere to write anything to
  HIPCHK(hipSetDevice(e->ctx->device));
  char* base = static_cast<char*>(d_scratch);
  u32* found = static_cast<u32*>(d_found);
  const u32* status = static_cast<const u32*>(d_status);
  const WeedKeysDev keys{static_cast<const uint8_t*>(d_ballots), static_cast<const uint8_t*>(d_board), (const u32*)e->d_tally_items,
                         (uint64_t)e->plan.stride, (uint64_t)n, (uint64_t)n_prior, K};
  const int cap = e->ctx->cus * 64;
  if (found) HIPCHK(hipMemsetAsync(found, 0, 3 * sizeof(u32), s));       // (n == 0 may come without: n_prior <= board_cap always fits)
  if (n) {
    unsigned long long* slots = reinterpret_cast<unsigned long long*>(base + L.table);
    u32* pos = reinterpret_cast<u32*>(base + L.pos);
    HIPCHK(hipMemsetAsync(slots, 0xff, (size_t)L.slots * sizeof(uint64_t), s));          // egw::EMPTY
    hipLaunchKernelGGL(k_weed_insert, dim3(grid_for(n_prior + n * K, cap)), dim3(WEED_NT), 0, s, keys, status, slots, L.slots, hash_seed, found);
    hipLaunchKernelGGL(k_weed_lookup, dim3(blocks_of(n)), dim3(WEED_NT), 0, s, keys, status, (const unsigned long long*)slots, L.slots, hash_seed,
                       static_cast<u32*>(d_dup_of), static_cast<u32*>(d_status_out), pos, found);
    if (d_board_count) {
      u32* tiles = reinterpret_cast<u32*>(base + L.tiles);
      u32* total_word = reinterpret_cast<u32*>(base + L.total_word);
      hipLaunchKernelGGL(k_weed_scan_tiles, dim3(L.n_tiles), dim3(WEED_NT), 0, s, (const u32*)pos, (u32)n, tiles);
      hipLaunchKernelGGL(k_weed_scan_tops, dim3(1), dim3(64), 0, s, L.n_tiles, tiles, K, (uint64_t)n_prior, (uint64_t)board_cap, total_word,
                         static_cast<unsigned long long*>(d_board_count), found);
      hipLaunchKernelGGL(k_weed_scan_apply, dim3(L.n_tiles), dim3(WEED_NT), 0, s, pos, (u32)n, (const u32*)tiles);
      hipLaunchKernelGGL(k_weed_copy, dim3(grid_for(n * K * 4, cap)), dim3(WEED_NT), 0, s, keys, (const u32*)pos, (const u32*)total_word,
                         static_cast<uint8_t*>(d_board), (uint64_t)board_cap);
    }
  } else if (d_board_count) {                                             // nothing to add: the count is n_prior
    hipLaunchKernelGGL(k_weed_scan_tops, dim3(1), dim3(64), 0, s, 0u, (u32*)nullptr, K, (uint64_t)n_prior, (uint64_t)board_cap, (u32*)nullptr,
                       static_cast<unsigned long long*>(d_board_count), found);
  }
  HIPCHK(hipGetLastError());
  return EG_OK;
}
static uint64_t weed_draw_seed() {
  std::random_device rd;
  return ((uint64_t)rd() << 32) ^ (uint64_t)rd();
}
// host buffers, staged as grouped_host stages them; the board is staged with room for every key of the batch when `appended` is given
static int weed_host(Engine* e, size_t n, const uint8_t* ballots, const uint32_t* status, size_t n_prior, const uint8_t* board, uint32_t* dup_of,
                     uint32_t* status_out, uint8_t* appended, size_t* n_appended) {
  if (n_appended) *n_appended = 0;
  TRY_(weed_check(e, n, n_prior, n_prior, ballots != nullptr, dup_of != nullptr, true, board != nullptr, false));
  if (appended && !n_appended) return fail(EG_ERR_BAD_ARG, "weed: null n_appended");
  HIPCHK(hipSetDevice(e->ctx->device));
  const size_t K = weed_keys_per_ballot(e), stride = e->plan.stride;
  const size_t board_cap = n_prior + (appended ? n * K : 0);
  HostStage st("weed"); TRY_(st.open());
  void *db, *dst = nullptr, *dboard, *scratch, *ddup, *dout;
  TRY_(st.put(&db, ballots, n * stride));
  if (status) TRY_(st.put(&dst, status, n * 4));
  TRY_(st.put(&dboard, nullptr, board_cap * egw::KEY_BYTES));             // room for the appended keys behind the caller's n_prior entries
  if (n_prior) HIPCHK(hipMemcpyAsync(dboard, board, n_prior * egw::KEY_BYTES, hipMemcpyHostToDevice, st.s));
  TRY_(st.put(&scratch, nullptr, weed_scratch_bytes(e, n, n_prior)));
  TRY_(st.put(&ddup, nullptr, n * 4));
  TRY_(st.put(&dout, nullptr, n * 4 + 32));           // status_out, then (8-byte aligned) the board count and the three counters
  char* tail = static_cast<char*>(dout) + (n * 4 + 7) / 8 * 8;
  unsigned long long* d_count = reinterpret_cast<unsigned long long*>(tail);
  u32* d_found = reinterpret_cast<u32*>(tail + 8);
  TRY_(weed_launch(e, n, db, dst, n_prior, dboard, board_cap, weed_draw_seed(), scratch, ddup, status_out ? dout : nullptr,
                   appended ? d_count : nullptr, d_found, st.s));
  u32 found[3] = {0, 0, 0};
  unsigned long long count = n_prior;
  if (n) TRY_(st.get(dup_of, ddup, n * 4));
  if (n && status_out) TRY_(st.get(status_out, dout, n * 4));
  TRY_(st.get(found, d_found, sizeof found));
  if (appended) TRY_(st.get(&count, d_count, sizeof count));
  TRY_(st.sync());
  if (appended && count > n_prior && count <= board_cap) {
    TRY_(st.get(appended, static_cast<char*>(dboard) + n_prior * egw::KEY_BYTES, (count - n_prior) * egw::KEY_BYTES));
    TRY_(st.sync());
    *n_appended = (size_t)(count - n_prior);
  }
  if (found[2]) return fail(EG_ERR_BAD_ARG, "weed: the table overflowed or the board has no room (" + std::to_string(found[2]) + "): discard the results");
  return EG_OK;
}
size_t eg_choice_weed_scratch_bytes(const eg_choice_params* p, size_t n, size_t n_prior) { return weed_scratch_bytes(p ? p->eng : nullptr, n, n_prior); }
size_t eg_qv_weed_scratch_bytes(const eg_qv_params* p, size_t n, size_t n_prior) { return weed_scratch_bytes(p ? p->eng : nullptr, n, n_prior); }
int eg_choice_weed_device(eg_choice_params* p, size_t n, const void* d_ballots, const void* d_status, size_t n_prior, void* d_board, size_t board_cap,
                          uint64_t hash_seed, void* d_scratch, void* d_dup_of, void* d_status_out, void* d_board_count, void* d_found, void* stream) {
  return weed_launch(p ? p->eng : nullptr, n, d_ballots, d_status, n_prior, d_board, board_cap, hash_seed, d_scratch, d_dup_of, d_status_out,
                     d_board_count, d_found, (hipStream_t)stream);
}
int eg_qv_weed_device(eg_qv_params* p, size_t n, const void* d_ballots, const void* d_status, size_t n_prior, void* d_board, size_t board_cap,
                      uint64_t hash_seed, void* d_scratch, void* d_dup_of, void* d_status_out, void* d_board_count, void* d_found, void* stream) {
  return weed_launch(p ? p->eng : nullptr, n, d_ballots, d_status, n_prior, d_board, board_cap, hash_seed, d_scratch, d_dup_of, d_status_out,
                     d_board_count, d_found, (hipStream_t)stream);
}
int eg_choice_weed(eg_choice_params* p, size_t n, const uint8_t* ballots, const uint32_t* status, size_t n_prior, const uint8_t* board,
                   uint32_t* dup_of, uint32_t* status_out, uint8_t* appended, size_t* n_appended) {
  return weed_host(p ? p->eng : nullptr, n, ballots, status, n_prior, board, dup_of, status_out, appended, n_appended);
}
int eg_qv_weed(eg_qv_params* p, size_t n, const uint8_t* ballots, const uint32_t* status, size_t n_prior, const uint8_t* board, uint32_t* dup_of,
               uint32_t* status_out, uint8_t* appended, size_t* n_appended) {
  return weed_host(p ? p->eng : nullptr, n, ballots, status, n_prior, board, dup_of, status_out, appended, n_appended);
}
// ---- weeding against a persistent board index (weed_index_kernels.cuh): the board's table is the caller's, a call costs O(batch) ------------
// Stateless with respect to the library like weeding itself: the index is the caller's device memory, as the roll and the node store are.
static int weed_index_check(const char* who, size_t n_prior, size_t board_cap, const void* d_board, const void* d_index) {
  const char* why = egw::refuse_indexed(0, n_prior, board_cap);
  if (!why && !d_index) why = "null index";
  if (!why && !d_board && n_prior) why = "null board with n_prior > 0";
  if (!why && (((uintptr_t)d_board | (uintptr_t)d_index) & 15u)) why = "index and board must be 16-byte aligned";
  return why ? fail(EG_ERR_BAD_ARG, std::string(who) + ": " + why) : EG_OK;
}
size_t eg_weed_index_bytes(size_t board_cap) { return egw::index_bytes(board_cap); }
int eg_weed_index_build_device(eg_ctx* c, size_t n_prior, const void* d_board, size_t board_cap, uint64_t index_seed, void* d_index, void* d_found,
                               void* stream) {
  TRY_(weed_index_check("weed index build", n_prior, board_cap, d_board, d_index));
  if (!d_found) return fail(EG_ERR_BAD_ARG, "weed index build: null found");
  if ((uintptr_t)d_found & 3u) return fail(EG_ERR_BAD_ARG, "weed index build: misaligned device pointer");
  TRY_(check_ctx("weed index build", c));
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  const uint64_t slots = egw::table_slots(board_cap);
  HIPCHK(hipMemsetAsync(d_index, 0xff, (size_t)slots * sizeof(u32), s));                  // egw::INDEX_EMPTY
  HIPCHK(hipMemsetAsync(d_found, 0, sizeof(u32), s));
  if (n_prior)
    hipLaunchKernelGGL(k_weed_index_add, dim3(grid_for(n_prior, c->cus * 64)), dim3(WEED_NT), 0, s, static_cast<const uint8_t*>(d_board), (uint64_t)0,
                       (uint64_t)n_prior, (const unsigned long long*)nullptr, (uint64_t)board_cap, static_cast<unsigned int*>(d_index), slots,
                       index_seed, static_cast<u32*>(d_found));
  HIPCHK(hipGetLastError());
  return EG_OK;
}
int eg_weed_index_find_device(eg_ctx* c, size_t n_q, const void* d_keys, size_t n_prior, const void* d_board, size_t board_cap, const void* d_index,
                              uint64_t index_seed, void* d_pos, void* stream) {
  if (n_q >= egw::N_LIMIT) return fail(EG_ERR_BAD_ARG, "weed index find: n_q is 2^31 or more");
  TRY_(weed_index_check("weed index find", n_prior, board_cap, d_board, d_index));
  if (n_q && !d_keys) return fail(EG_ERR_BAD_ARG, "weed index find: null keys");
  if (n_q && !d_pos) return fail(EG_ERR_BAD_ARG, "weed index find: null pos");
  if ((uintptr_t)d_keys & 15u) return fail(EG_ERR_BAD_ARG, "weed index find: keys must be 16-byte aligned");
  if ((uintptr_t)d_pos & 3u) return fail(EG_ERR_BAD_ARG, "weed index find: misaligned device pointer");
  TRY_(check_ctx("weed index find", c));
  if (n_q == 0) return EG_OK;
  HIPCHK(hipSetDevice(c->device));
  const WeedFindKeysDev keys{static_cast<const uint8_t*>(d_keys), static_cast<const uint8_t*>(d_board), (uint64_t)n_q, (uint64_t)n_prior};
  hipLaunchKernelGGL(k_weed_index_find, dim3(grid_for(n_q, c->cus * 64)), dim3(WEED_NT), 0, (hipStream_t)stream, keys,
                     static_cast<const unsigned int*>(d_index), egw::table_slots(board_cap), index_seed, static_cast<u32*>(d_pos));
  HIPCHK(hipGetLastError());
  return EG_OK;
}
static size_t weed_indexed_scratch_bytes(const Engine* e, size_t n) {
  if (!e || !e->weed_keys_ok || n >= egw::N_LIMIT || egw::refuse_indexed_keys(n, weed_keys_per_ballot(e))) return 0;
  return egw::layout_indexed(n, weed_keys_per_ballot(e)).total;
}
static int weed_indexed_launch(Engine* e, size_t n, const void* d_ballots, const void* d_status, size_t n_prior, void* d_board, size_t board_cap,
                               void* d_index, uint64_t index_seed, uint64_t hash_seed, void* d_scratch, void* d_dup_of, void* d_status_out,
                               void* d_board_count, void* d_found, hipStream_t s) {
  if (((uintptr_t)d_ballots | (uintptr_t)d_board | (uintptr_t)d_scratch | (uintptr_t)d_index) & 15u)
    return fail(EG_ERR_BAD_ARG, "weed: ballots, board, index and scratch must be 16-byte aligned");
  if (((uintptr_t)d_status | (uintptr_t)d_dup_of | (uintptr_t)d_status_out | (uintptr_t)d_found) & 3u || ((uintptr_t)d_board_count & 7u))
    return fail(EG_ERR_BAD_ARG, "weed: misaligned device pointer");
  const char* why = egw::refuse_indexed(n, n_prior, board_cap);
  if (!why && !d_index) why = "null index";
  if (!why && !d_board && n_prior) why = "null board with n_prior > 0";
  if (why) return fail(EG_ERR_BAD_ARG, std::string("weed: ") + why);
  // the board is outside the key limit here: the stateless rules are asked about the batch alone
  TRY_(weed_check(e, n, 0, board_cap, d_ballots != nullptr, d_dup_of != nullptr, d_found != nullptr, d_board != nullptr, d_board_count != nullptr));
  const u32 K = weed_keys_per_ballot(e);
  const egw::Layout L = egw::layout_indexed(n, K);
  if (L.total && !d_scratch) return fail(EG_ERR_BAD_ARG, "weed: null scratch (eg_*_weed_indexed_scratch_bytes says how much)");
  if (!d_found && !d_board_count) return EG_OK;                          // n == 0 and nowhere to write anything to
  HIPCHK(hipSetDevice(e->ctx->device));
  char* base = static_cast<char*>(d_scratch);
  u32* found = static_cast<u32*>(d_found);
  const u32* status = static_cast<const u32*>(d_status);
  const WeedKeysDev keys{static_cast<const uint8_t*>(d_ballots), static_cast<const uint8_t*>(d_board), (const u32*)e->d_tally_items,
                         (uint64_t)e->plan.stride, (uint64_t)n, (uint64_t)n_prior, K};
  WeedKeysDev batch_keys = keys;
  batch_keys.n_prior = 0;                                                 // the batch table: lanes and references of the batch alone
  const int cap = e->ctx->cus * 64;
  const uint64_t index_slots = egw::table_slots(board_cap);
  if (found) HIPCHK(hipMemsetAsync(found, 0, 3 * sizeof(u32), s));
  if (n) {
    unsigned long long* slots = reinterpret_cast<unsigned long long*>(base + L.table);
    u32* pos = reinterpret_cast<u32*>(base + L.pos);
    HIPCHK(hipMemsetAsync(slots, 0xff, (size_t)L.slots * sizeof(uint64_t), s));          // egw::EMPTY
    hipLaunchKernelGGL(k_weed_insert, dim3(grid_for(n * K, cap)), dim3(WEED_NT), 0, s, batch_keys, status, slots, L.slots, hash_seed, found);
    hipLaunchKernelGGL(k_weed_lookup_indexed, dim3(blocks_of(n)), dim3(WEED_NT), 0, s, keys, status, static_cast<const unsigned int*>(d_index),
                       index_slots, index_seed, (const unsigned long long*)slots, L.slots, hash_seed, static_cast<u32*>(d_dup_of),
                       static_cast<u32*>(d_status_out), pos, found);
    if (d_board_count) {
      u32* tiles = reinterpret_cast<u32*>(base + L.tiles);
      u32* total_word = reinterpret_cast<u32*>(base + L.total_word);
      hipLaunchKernelGGL(k_weed_scan_tiles, dim3(L.n_tiles), dim3(WEED_NT), 0, s, (const u32*)pos, (u32)n, tiles);
      hipLaunchKernelGGL(k_weed_scan_tops, dim3(1), dim3(64), 0, s, L.n_tiles, tiles, K, (uint64_t)n_prior, (uint64_t)board_cap, total_word,
                         static_cast<unsigned long long*>(d_board_count), found);
      hipLaunchKernelGGL(k_weed_scan_apply, dim3(L.n_tiles), dim3(WEED_NT), 0, s, pos, (u32)n, (const u32*)tiles);
      hipLaunchKernelGGL(k_weed_copy, dim3(grid_for(n * K * 4, cap)), dim3(WEED_NT), 0, s, keys, (const u32*)pos, (const u32*)total_word,
                         static_cast<uint8_t*>(d_board), (uint64_t)board_cap);
      // what has just been appended -> the index; the count is on the device, so the grid is sized by the most that can have been
      hipLaunchKernelGGL(k_weed_index_add, dim3(grid_for(n * K, cap)), dim3(WEED_NT), 0, s, static_cast<const uint8_t*>(d_board), (uint64_t)n_prior,
                         (uint64_t)n_prior, static_cast<const unsigned long long*>(d_board_count), (uint64_t)board_cap,
                         static_cast<unsigned int*>(d_index), index_slots, index_seed, found + 2);
    }
  } else if (d_board_count) {                                             // nothing to add: the count is n_prior
    hipLaunchKernelGGL(k_weed_scan_tops, dim3(1), dim3(64), 0, s, 0u, (u32*)nullptr, K, (uint64_t)n_prior, (uint64_t)board_cap, (u32*)nullptr,
                       static_cast<unsigned long long*>(d_board_count), found);
  }
  HIPCHK(hipGetLastError());
  return EG_OK;
}
size_t eg_choice_weed_indexed_scratch_bytes(const eg_choice_params* p, size_t n) { return weed_indexed_scratch_bytes(p ? p->eng : nullptr, n); }
size_t eg_qv_weed_indexed_scratch_bytes(const eg_qv_params* p, size_t n) { return weed_indexed_scratch_bytes(p ? p->eng : nullptr, n); }
int eg_choice_weed_indexed_device(eg_choice_params* p, size_t n, const void* d_ballots, const void* d_status, size_t n_prior, void* d_board,
                                  size_t board_cap, void* d_index, uint64_t index_seed, uint64_t hash_seed, void* d_scratch, void* d_dup_of,
                                  void* d_status_out, void* d_board_count, void* d_found, void* stream) {
  return weed_indexed_launch(p ? p->eng : nullptr, n, d_ballots, d_status, n_prior, d_board, board_cap, d_index, index_seed, hash_seed, d_scratch,
                             d_dup_of, d_status_out, d_board_count, d_found, (hipStream_t)stream);
}
int eg_qv_weed_indexed_device(eg_qv_params* p, size_t n, const void* d_ballots, const void* d_status, size_t n_prior, void* d_board, size_t board_cap,
                              void* d_index, uint64_t index_seed, uint64_t hash_seed, void* d_scratch, void* d_dup_of, void* d_status_out,
                              void* d_board_count, void* d_found, void* stream) {
  return weed_indexed_launch(p ? p->eng : nullptr, n, d_ballots, d_status, n_prior, d_board, board_cap, d_index, index_seed, hash_seed, d_scratch,
                             d_dup_of, d_status_out, d_board_count, d_found, (hipStream_t)stream);
}
// builds the wide comb tables now (synchronously, ~12 GB each for G and K) instead of inside the first large verify call
static int prepare_wide(Engine* e) {
  HIPCHK(hipSetDevice(e->ctx->device));
  HIPCHK(hipDeviceSynchronize());
  const int rc = ensure_big_tables(e, e->ctx->stream);
  if (rc) return rc;
  if (e->ctx->big_bits && !engine_wide(e)) return fail(EG_ERR_NOMEM, "the wide comb tables do not fit the device memory");
  return EG_OK;
}
int eg_choice_prepare_wide_tables(eg_choice_params* p) { EG_LOCK_P(p); return p ? prepare_wide(p->eng) : fail(EG_ERR_BAD_ARG, "null"); }
int eg_qv_prepare_wide_tables(eg_qv_params* p) { EG_LOCK_P(p); return p ? prepare_wide(p->eng) : fail(EG_ERR_BAD_ARG, "null"); }
int eg_choice_tally_reset(eg_choice_params* p) { EG_LOCK_P(p); if (!p) return fail(EG_ERR_BAD_ARG, "null"); EG_WAIT_JSON(p->eng); return tally_reset(p->eng, p->eng->ctx->stream, true); }
int eg_choice_tally_reset_async(eg_choice_params* p, void* stream) { EG_LOCK_P(p); if (!p) return fail(EG_ERR_BAD_ARG, "null"); EG_WAIT_JSON(p->eng); return tally_reset(p->eng, (hipStream_t)stream, false); }
int eg_choice_tally_add(eg_choice_params* p, const uint8_t* in) { EG_LOCK_P(p);
  if (!p || !in) return fail(EG_ERR_BAD_ARG, "bad argument");
  EG_WAIT_JSON(p->eng);
  return engine_tally_add(p->eng, in);
}
int eg_qv_tally_add(eg_qv_params* p, const uint8_t* in) { EG_LOCK_P(p);
  if (!p || !in) return fail(EG_ERR_BAD_ARG, "bad argument");
  EG_WAIT_JSON(p->eng);
  return engine_tally_add(p->eng, in);
}
int eg_choice_tally_encode(eg_choice_params* p, uint8_t* out) { EG_LOCK_P(p);
  if (!p || !out) return fail(EG_ERR_BAD_ARG, "bad argument");
  EG_WAIT_JSON(p->eng);
  return engine_tally_encode(p->eng, out);
}

// ---- batch tier: quadratic voting --------------------------------------------------------------------------------------------
int eg_qv_params_create(eg_ctx* c, const uint8_t pk[32], int n_options, uint64_t credits, eg_qv_params** out) { EG_LOCK(c);
  if (!c || !pk || !out) return fail(EG_ERR_BAD_ARG, "bad argument");
  if (n_options < 1 || n_options > 256 || credits < 1 || credits > 100000) return fail(EG_ERR_BAD_ARG, "options in 1..256, credits in 1..100000");
  Engine* e = nullptr;
  TRY(engine_create(c, eghost::build_qv_plan(n_options, credits), pk, n_options, &e));
  *out = new eg_qv_params{e, n_options, credits, eghost::qv_shape(n_options, credits)};
  return EG_OK;
}
void eg_qv_params_destroy(eg_qv_params* p) { params_destroy(p); }
size_t eg_qv_ballot_size(const eg_qv_params* p) { return p ? p->shape.ballot_size : 0; }
int eg_verify_qv_batch(eg_qv_params* p, size_t n, const uint8_t* ballots, uint32_t* status, uint8_t* tally_out) { EG_LOCK_P(p);
  if (!p || (n && (!ballots || !status))) return fail(EG_ERR_BAD_ARG, "bad argument");
  EG_WAIT_JSON(p->eng);
  return engine_verify_host(p->eng, n, ballots, status, tally_out);
}
int eg_verify_qv_batch_device(eg_qv_params* p, size_t n, const void* d_ballots, void* d_status, void* stream) { EG_LOCK_P(p);
  if (!p || (n && (!d_ballots || !d_status))) return fail(EG_ERR_BAD_ARG, "bad argument");
  EG_WAIT_JSON(p->eng);
  HIPCHK(hipSetDevice(p->eng->ctx->device));
  return engine_verify_device(p->eng, n, d_ballots, d_status, (hipStream_t)stream);
}
int eg_qv_tally_reset(eg_qv_params* p) { EG_LOCK_P(p); if (!p) return fail(EG_ERR_BAD_ARG, "null"); EG_WAIT_JSON(p->eng); return tally_reset(p->eng, p->eng->ctx->stream, true); }
int eg_qv_tally_reset_async(eg_qv_params* p, void* stream) { EG_LOCK_P(p); if (!p) return fail(EG_ERR_BAD_ARG, "null"); EG_WAIT_JSON(p->eng); return tally_reset(p->eng, (hipStream_t)stream, false); }
int eg_qv_tally_encode(eg_qv_params* p, uint8_t* out) { EG_LOCK_P(p);
  if (!p || !out) return fail(EG_ERR_BAD_ARG, "bad argument");
  EG_WAIT_JSON(p->eng);
  return engine_tally_encode(p->eng, out);
}

// ---- small-batch tier: the same arguments and meaning as the batch entries, for at most EG_SMALL_BATCH_MAX ballots per call ----------
extern "C++" {
template <class Params>
static int verify_small_host(std::unique_lock<std::recursive_mutex>& lk_, Params* p, size_t n, const uint8_t* ballots, uint32_t* status, uint8_t* tally_out) {
  if (n > EG_SMALL_BATCH_MAX) return fail(EG_ERR_BAD_ARG, "more than EG_SMALL_BATCH_MAX ballots: use the batch entry");
  if (!p || (n && (!ballots || !status))) return fail(EG_ERR_BAD_ARG, "bad argument");
  EG_WAIT_JSON(p->eng);
  return engine_verify_host(p->eng, n, ballots, status, tally_out, true);
}
template <class Params>
static int verify_small_dev(std::unique_lock<std::recursive_mutex>& lk_, Params* p, size_t n, const void* d_ballots, void* d_status, void* stream) {
  if (n > EG_SMALL_BATCH_MAX) return fail(EG_ERR_BAD_ARG, "more than EG_SMALL_BATCH_MAX ballots: use the batch entry");
  if (!p || (n && (!d_ballots || !d_status))) return fail(EG_ERR_BAD_ARG, "bad argument");
  EG_WAIT_JSON(p->eng);
  HIPCHK(hipSetDevice(p->eng->ctx->device));
  return engine_verify_small_device(p->eng, n, d_ballots, d_status, (hipStream_t)stream);
}
}  // extern "C++"
int eg_verify_choice_small(eg_choice_params* p, size_t n, const uint8_t* ballots, uint32_t* status, uint8_t* tally_out) { EG_LOCK_P(p);
  return verify_small_host(lk_, p, n, ballots, status, tally_out);
}
int eg_verify_choice_small_device(eg_choice_params* p, size_t n, const void* d_ballots, void* d_status, void* stream) { EG_LOCK_P(p);
  return verify_small_dev(lk_, p, n, d_ballots, d_status, stream);
}
int eg_verify_qv_small(eg_qv_params* p, size_t n, const uint8_t* ballots, uint32_t* status, uint8_t* tally_out) { EG_LOCK_P(p);
  return verify_small_host(lk_, p, n, ballots, status, tally_out);
}
int eg_verify_qv_small_device(eg_qv_params* p, size_t n, const void* d_ballots, void* d_status, void* stream) { EG_LOCK_P(p);
  return verify_small_dev(lk_, p, n, d_ballots, d_status, stream);
}

// ---- batch tier, several GPUs in ONE process (the `device_mask` of the batch entry; examples/voting.rs:179-213 is one
// single-threaded host process) ------------------------------------------------------------------------------------------------
// per_device[d] is a params object of the same election created on its own context (normally one context per GPU).  The batch is
// cut into contiguous slabs, slab d = [n d / n_dev, n (d + 1) / n_dev) (the split of elastic_elgamal_amd/distributed.py:
// shard_range), and one host thread per params object runs the ordinary host entry on its slab: its own device, streams, uploads and
// running tally.  The per-slab tallies (64 n_options bytes each) are merged on the host side of the ABI with the element addition
// of the primitive tier on the first context - in one process there is nothing for RCCL to do.
extern "C++" {
// the checks every multi entry shares: n_dev objects, all different, all of one election
template <class Params>
static int multi_check(Params* const* per_device, int n_dev) {
  if (!per_device || n_dev < 1 || n_dev > 64) return fail(EG_ERR_BAD_ARG, "bad argument");
  for (int d = 0; d < n_dev; ++d) {
    if (!per_device[d]) return fail(EG_ERR_BAD_ARG, "null params object");
    for (int k = 0; k < d; ++k)
      if (per_device[k] == per_device[d]) return fail(EG_ERR_BAD_ARG, "the same params object given twice: one object (and context) per slab");
    const eghost::Plan &A = per_device[0]->eng->plan, &B = per_device[d]->eng->plan;
    if (B.stride != A.stride || per_device[d]->n_options != per_device[0]->n_options || B.tally_slots.size() != A.tally_slots.size() ||
        memcmp(per_device[d]->eng->key_bytes, per_device[0]->eng->key_bytes, 32) != 0)
      return fail(EG_ERR_BAD_ARG, "params objects of different elections");
  }
  return EG_OK;
}
// One host thread per slab (the caller's thread takes slab 0), nothing escapes the C ABI: an exception inside a slab's work becomes that
// slab's error code.
template <class Work>
static void multi_run(int n_dev, std::vector<int>& rcs, std::vector<std::string>& errs, Work work) {
  auto guarded = [&](int d) {
    try {
      rcs[d] = work(d);
      if (rcs[d]) errs[d] = g_err;          // eg_last_error is per thread: carry the text over to the caller's
    } catch (const std::bad_alloc&) { rcs[d] = EG_ERR_NOMEM; errs[d] = "out of host memory";
    } catch (const std::exception& ex) { rcs[d] = EG_ERR_HIP; errs[d] = std::string("exception: ") + ex.what();
    } catch (...) { rcs[d] = EG_ERR_HIP; errs[d] = "unknown exception"; }
  };
  std::vector<std::thread> threads;
  int started = 0;
  try {
    for (int d = 1; d < n_dev; ++d) { threads.emplace_back(guarded, d); started = d; }
  } catch (const std::exception&) {          // no thread for a slab (resource limits): the caller's thread takes it over
    for (int d = started + 1; d < n_dev; ++d) guarded(d);
  }
  guarded(0);
  for (auto& t : threads) t.join();
}
// A multi call HOLDS its params objects from its first check to its merge or roll-back (Engine::long_call_mu + Engine::reserved): it waits
// for a one-shot JSON call that is running on any of them, REFUSES when an explicitly opened JSON stream owns one (nothing has been touched
// at that point: the stream's tally share and its set-aside running tally are as they were), and every call of another thread on a held
// object waits until the multi call is over (EG_WAIT_LONG_ONLY) - so nothing can interleave between save() and restore() (ADVICE r5, medium:
// a snapshot taken in the middle of another call, or put back over one, lost or misattributed ballots).  The mutexes are taken in address
// order, so two multi calls over the same objects in different orders cannot deadlock.
template <class Params>
struct MultiHold {
  std::vector<Engine*> held;
  int acquire(Params* const* per_device, int n_dev) {
    std::vector<Engine*> order;
    for (int d = 0; d < n_dev; ++d) order.push_back(per_device[d]->eng);
    std::sort(order.begin(), order.end(), std::less<Engine*>());
    for (Engine* e : order) {
      e->long_call_mu.lock();
      std::lock_guard<std::recursive_mutex> g(e->ctx->mu);
      if (e->stream_open) {            // (a one-shot stream cannot be: its call holds long_call_mu)
        e->long_call_mu.unlock();
        release();
        return fail(EG_ERR_BAD_ARG, "a JSON stream is open on one of the params objects (eg_verify_json_end or _abort it first)");
      }
      e->reserved = true;
      held.push_back(e);
    }
    return EG_OK;
  }
  void release() {
    for (auto it = held.rbegin(); it != held.rend(); ++it) {
      { std::lock_guard<std::recursive_mutex> g((*it)->ctx->mu); (*it)->reserved = false; }
      (*it)->long_call_mu.unlock();
    }
    held.clear();
  }
  ~MultiHold() { release(); }
};
// The running tallies before a multi call and the way back to them: a multi call that fails in ANY slab leaves every running tally as it
// found it (a host that retries the batch must not count slabs twice).  The tallies stay ON their devices (Engine::tally_saved3: a
// device-to-device copy of 2n points, no allocation, no encoding), and nothing here drains a device (round 5 did, twice per GPU and call):
// save() orders the copy after the engine's last asynchronous call with an event (Engine::last_done) and leaves an event behind
// (Engine::saved_ev) that the slab's stream waits for; restore() waits for the slab's own stream.  The engines are held (MultiHold), so
// no other call can touch the tallies in between.
template <class Params>
struct TallyRollback {
  Params* const* per_device; int n_dev; size_t bytes;
  std::vector<hipStream_t> slab_stream;      // device form: the stream slab d was enqueued on; host form: empty (the contexts' own streams)
  int save() {
    if (!bytes) return EG_OK;
    for (int d = 0; d < n_dev; ++d) {
      Engine* e = per_device[d]->eng;
      std::lock_guard<std::recursive_mutex> g(e->ctx->mu);
      HIPCHK(hipSetDevice(e->ctx->device));
      hipStream_t s = e->ctx->stream;
      if (e->last_used) HIPCHK(hipStreamWaitEvent(s, e->last_done, 0));      // earlier _device calls on caller streams land in the tally that is set aside
      HIPCHK(hipMemcpyAsync(e->tally_saved3, e->tally, e->plan.tally_slots.size() * PT_WORDS * sizeof(u32), hipMemcpyDeviceToDevice, s));
      HIPCHK(hipEventRecord(e->saved_ev, s));
    }
    return EG_OK;
  }
  // the slab's work starts after the copy above (device form; the host form runs on the context's own stream, behind the copy)
  int order_slab_after_save(int d, hipStream_t s) {
    if (!bytes) return EG_OK;
    HIPCHK(hipStreamWaitEvent(s, per_device[d]->eng->saved_ev, 0));
    return EG_OK;
  }
  int encoded_before(int d, uint8_t* out) {
    Engine* e = per_device[d]->eng;
    std::lock_guard<std::recursive_mutex> g(e->ctx->mu);
    HIPCHK(hipSetDevice(e->ctx->device));
    return engine_tally_encode_from(e, e->tally_saved3, out, false);
  }
  int restore() {
    if (!bytes) return EG_OK;
    int first = EG_OK;
    for (int d = 0; d < n_dev; ++d) {
      Engine* e = per_device[d]->eng;
      std::lock_guard<std::recursive_mutex> g(e->ctx->mu);
      hipStream_t s = e->ctx->stream;
      hipError_t he = hipSetDevice(e->ctx->device);
      // whatever the failed slab still has in flight sits on its stream (engine_verify_device joins its work sets back into it on every
      // way out) or, host form, on the context's own: the copy back goes behind it
      if (he == hipSuccess && !slab_stream.empty() && slab_stream[d] != s) {
        he = hipEventRecord(e->last_done, slab_stream[d]);
        if (he == hipSuccess) he = hipStreamWaitEvent(s, e->last_done, 0);
      }
      if (he == hipSuccess) he = hipMemcpyAsync(e->tally, e->tally_saved3, e->plan.tally_slots.size() * PT_WORDS * sizeof(u32), hipMemcpyDeviceToDevice, s);
      if (he == hipSuccess && e->n_sets == 2)        // a share of the failed call that set 1 still holds must not reach the tally later (this call holds the engine)
        hipLaunchKernelGGL(k_tally_init, dim3(blocks_of(e->plan.tally_slots.size())), dim3(NT), 0, s, e->set[1].tally, (int)e->plan.tally_slots.size());
      if (he == hipSuccess) he = hipEventRecord(e->last_done, s);
      if (he == hipSuccess) { e->last_used = true; he = hipStreamSynchronize(s); }
      if (he != hipSuccess && !first) first = EG_ERR_HIP;
    }
    return first;
  }
};
template <class Params>
static int multi_fail(Params* const* per_device, int n_dev, const std::vector<int>& rcs, const std::vector<std::string>& errs, TallyRollback<Params>& rb) {
  for (int d = 0; d < n_dev; ++d)
    if (rcs[d]) {
      const bool back = rb.restore() == EG_OK;
      return fail(rcs[d], "slab " + std::to_string(d) + " of " + std::to_string(n_dev) + ": " + errs[d] +
                              (back ? " (every running tally is as it was before the call)" : " (AND the running tallies could not be restored: reset them)"));
    }
  return EG_OK;
}
// merges per-slab tally encodings (host) into out with the element addition of the primitive tier on the first context
template <class Params>
static int multi_merge(Params* const* per_device, int n_dev, const std::vector<std::vector<uint8_t>>& tallies, size_t tally_bytes, uint8_t* out) {
  if (!tally_bytes) return EG_OK;
  memcpy(out, tallies[0].data(), tally_bytes);
  std::vector<uint8_t> ok(tally_bytes / 32);
  for (int d = 1; d < n_dev; ++d) {
    TRY(eg_point_add_batch(per_device[0]->eng->ctx, tally_bytes / 32, out, tallies[d].data(), 0, out, ok.data()));
    for (uint8_t o : ok) if (!o) return fail(EG_ERR_HIP, "the tally of slab " + std::to_string(d) + " does not decode");
  }
  return EG_OK;
}
// the entry points' bodies without their wait for long calls: what a multi call, which HOLDS the objects, runs on its slabs
template <class Params>
static int held_verify_host(Params* p, size_t n, const uint8_t* ballots, uint32_t* status, uint8_t* tally_out) { EG_LOCK_P(p);
  return engine_verify_host(p->eng, n, ballots, status, tally_out);
}
template <class Params>
static int held_verify_device(Params* p, size_t n, const void* d_ballots, void* d_status, hipStream_t s) { EG_LOCK_P(p);
  HIPCHK(hipSetDevice(p->eng->ctx->device));
  return engine_verify_device(p->eng, n, d_ballots, d_status, s);
}
template <class Params>
static int verify_batch_multi(Params* const* per_device, int n_dev, size_t n, const uint8_t* ballots, uint32_t* status, uint8_t* tally_out) {
  TRY(multi_check(per_device, n_dev));
  KeepDevice keep;
  if (n && (!ballots || !status)) return fail(EG_ERR_BAD_ARG, "bad argument");
  MultiHold<Params> hold;
  TRY(hold.acquire(per_device, n_dev));
  const size_t stride = per_device[0]->eng->plan.stride;
  const size_t tally_bytes = (size_t)per_device[0]->eng->plan.tally_slots.size() * 32;
  std::vector<std::vector<uint8_t>> tallies(n_dev, std::vector<uint8_t>(tally_bytes));
  std::vector<int> rcs(n_dev, EG_OK);
  std::vector<std::string> errs(n_dev);
  TallyRollback<Params> rb{per_device, n_dev, tally_bytes, {}};
  TRY(rb.save());
  multi_run(n_dev, rcs, errs, [&](int d) {
    const size_t b = n * (size_t)d / (size_t)n_dev, e = n * (size_t)(d + 1) / (size_t)n_dev;
    return held_verify_host(per_device[d], e - b, ballots + b * stride, status + b, tally_out ? tallies[d].data() : nullptr);
  });
  TRY(multi_fail(per_device, n_dev, rcs, errs, rb));
  if (tally_out && tally_bytes) {
    const int rc = multi_merge(per_device, n_dev, tallies, tally_bytes, tally_out);
    if (rc) { const std::string why = g_err; (void)rb.restore(); return fail(rc, why); }
  }
  return EG_OK;
}
// The same with every slab ALREADY RESIDENT on its GPU: d_ballots[d] / d_status[d] are device pointers on per_device[d]'s device, n_per_dev[d]
// ballots each, streams[d] (may be NULL = all null streams) a stream of that device.  One host thread per slab enqueues
// eg_verify_*_batch_device and waits for its stream, so that the call returns with every verdict written and every running tally advanced;
// no byte of a ballot crosses PCIe or xGMI.
template <class Params>
static int verify_batch_multi_device(Params* const* per_device, int n_dev, const size_t* n_per_dev, const void* const* d_ballots,
                                     void* const* d_status, void* const* streams, uint8_t* tally_out) {
  TRY(multi_check(per_device, n_dev));
  KeepDevice keep;
  if (!n_per_dev || !d_ballots || !d_status) return fail(EG_ERR_BAD_ARG, "bad argument");
  for (int d = 0; d < n_dev; ++d)
    if (n_per_dev[d] && (!d_ballots[d] || !d_status[d])) return fail(EG_ERR_BAD_ARG, "null device pointer for a non-empty slab");
  MultiHold<Params> hold;
  TRY(hold.acquire(per_device, n_dev));
  const size_t tally_bytes = (size_t)per_device[0]->eng->plan.tally_slots.size() * 32;
  std::vector<int> rcs(n_dev, EG_OK);
  std::vector<std::string> errs(n_dev);
  TallyRollback<Params> rb{per_device, n_dev, tally_bytes, std::vector<hipStream_t>(n_dev, nullptr)};
  for (int d = 0; d < n_dev; ++d) rb.slab_stream[d] = streams ? (hipStream_t)streams[d] : nullptr;
  TRY(rb.save());
  multi_run(n_dev, rcs, errs, [&](int d) {
    hipStream_t s = rb.slab_stream[d];
    HIPCHK(hipSetDevice(per_device[d]->eng->ctx->device));
    TRY(rb.order_slab_after_save(d, s));
    TRY(held_verify_device(per_device[d], n_per_dev[d], d_ballots[d], d_status[d], s));
    HIPCHK(hipStreamSynchronize(s));
    return (int)EG_OK;
  });
  TRY(multi_fail(per_device, n_dev, rcs, errs, rb));
  if (tally_out && tally_bytes) {
    // the batch's own tally = (running tally after) - (running tally before), slab by slab, merged: all on 64 n_options bytes per device
    std::vector<std::vector<uint8_t>> tallies(n_dev, std::vector<uint8_t>(tally_bytes));
    std::vector<uint8_t> ok(tally_bytes / 32), before(tally_bytes);
    int rc = EG_OK;
    for (int d = 0; d < n_dev && !rc; ++d) {
      { std::lock_guard<std::recursive_mutex> g(per_device[d]->eng->ctx->mu);       // (every slab's stream has been waited for above)
        rc = hipSetDevice(per_device[d]->eng->ctx->device) == hipSuccess ? engine_tally_encode_from(per_device[d]->eng, per_device[d]->eng->tally, tallies[d].data(), false)
                                                                         : fail(EG_ERR_HIP, "hipSetDevice"); }
      if (!rc) rc = rb.encoded_before(d, before.data());
      if (!rc) rc = eg_point_add_batch(per_device[d]->eng->ctx, tally_bytes / 32, tallies[d].data(), before.data(), 1, tallies[d].data(), ok.data());
      if (!rc) for (uint8_t o : ok) if (!o) rc = fail(EG_ERR_HIP, "the tally of slab " + std::to_string(d) + " does not decode");
    }
    if (!rc) rc = multi_merge(per_device, n_dev, tallies, tally_bytes, tally_out);
    if (rc) { const std::string why = g_err; (void)rb.restore(); return fail(rc, why); }
  }
  return EG_OK;
}
// sum of the RUNNING tallies of the params objects (each keeps the tally of the slabs it verified); the objects are held while they are
// read, so the sum is the tally of whole calls only
template <class Params>
static int tally_encode_multi(Params* const* per_device, int n_dev, uint8_t* out) {
  TRY(multi_check(per_device, n_dev));
  KeepDevice keep;
  if (!out) return fail(EG_ERR_BAD_ARG, "bad argument");
  MultiHold<Params> hold;
  TRY(hold.acquire(per_device, n_dev));
  const size_t tally_bytes = (size_t)per_device[0]->eng->plan.tally_slots.size() * 32;
  std::vector<std::vector<uint8_t>> tallies(n_dev, std::vector<uint8_t>(tally_bytes));
  for (int d = 0; d < n_dev; ++d) {
    Params* p = per_device[d];
    EG_LOCK_P(p);
    TRY(engine_tally_encode(p->eng, tallies[d].data()));
  }
  return multi_merge(per_device, n_dev, tallies, tally_bytes, out);
}
}  // extern "C++"
int eg_verify_choice_batch_multi(eg_choice_params* const* per_device, int n_dev, size_t n, const uint8_t* ballots, uint32_t* status,
                                 uint8_t* tally_out) {
  return verify_batch_multi(per_device, n_dev, n, ballots, status, tally_out);
}
int eg_verify_qv_batch_multi(eg_qv_params* const* per_device, int n_dev, size_t n, const uint8_t* ballots, uint32_t* status,
                             uint8_t* tally_out) {
  return verify_batch_multi(per_device, n_dev, n, ballots, status, tally_out);
}
int eg_verify_choice_batch_multi_device(eg_choice_params* const* per_device, int n_dev, const size_t* n_per_dev, const void* const* d_ballots,
                                        void* const* d_status, void* const* streams, uint8_t* tally_out) {
  return verify_batch_multi_device(per_device, n_dev, n_per_dev, d_ballots, d_status, streams, tally_out);
}
int eg_verify_qv_batch_multi_device(eg_qv_params* const* per_device, int n_dev, const size_t* n_per_dev, const void* const* d_ballots,
                                    void* const* d_status, void* const* streams, uint8_t* tally_out) {
  return verify_batch_multi_device(per_device, n_dev, n_per_dev, d_ballots, d_status, streams, tally_out);
}
int eg_choice_tally_encode_multi(eg_choice_params* const* per_device, int n_dev, uint8_t* out) { return tally_encode_multi(per_device, n_dev, out); }
int eg_qv_tally_encode_multi(eg_qv_params* const* per_device, int n_dev, uint8_t* out) { return tally_encode_multi(per_device, n_dev, out); }

// ---- PublicKey::verify_zero / verify_bool / verify_range in batches ---------------------------------------
int eg_proof_params_create(eg_ctx* c, const uint8_t pk[32], int kind, uint64_t upper_bound, eg_proof_params** out) { EG_LOCK(c);
  if (!c || !pk || !out) return fail(EG_ERR_BAD_ARG, "bad argument");
  Engine* e = nullptr;
  size_t item = 0;
  if (kind == EG_PROOF_ZERO) { TRY(engine_create(c, eghost::build_zero_plan(), pk, 0, &e)); item = 128; }
  else if (kind == EG_PROOF_BOOL) { TRY(engine_create(c, eghost::build_bool_plan(), pk, 0, &e)); item = 160; }
  else if (kind == EG_PROOF_RANGE) {
    if (upper_bound < 2 || upper_bound > 1000000) return fail(EG_ERR_BAD_ARG, "upper_bound must be in 2..1000000");
    TRY(engine_create(c, eghost::build_range_plan(upper_bound, &item), pk, 0, &e));
  } else return fail(EG_ERR_BAD_ARG, "unknown proof kind");
  *out = new eg_proof_params{e, kind, item};
  if (kind == EG_PROOF_BOOL) (*out)->range.rings = {{2, 1}};
  if (kind == EG_PROOF_RANGE) { (*out)->upper_bound = upper_bound; (*out)->range = eghost::optimal_range(upper_bound); }
  return EG_OK;
}
int eg_share_params_create(eg_ctx* c, const uint8_t shared_key[32], uint64_t shares, uint64_t threshold, uint64_t index,
                           const uint8_t participant_key[32], eg_proof_params** out) { EG_LOCK(c);
  if (!c || !shared_key || !participant_key || !out) return fail(EG_ERR_BAD_ARG, "bad argument");
  if (shares < 1 || threshold < 1 || threshold > shares || index >= shares) return fail(EG_ERR_BAD_ARG, "bad sharing parameters");
  Engine* e = nullptr;
  TRY(engine_create(c, eghost::build_share_plan(shares, threshold, shared_key, index), participant_key, 0, &e));
  *out = new eg_proof_params{e, EG_PROOF_SHARE, 128};
  return EG_OK;
}
int eg_sumsq_params_create(eg_ctx* c, const uint8_t pk[32], int n_values, const char* label, size_t label_len, eg_proof_params** out) { EG_LOCK(c);
  if (!c || !pk || !out || (!label && label_len)) return fail(EG_ERR_BAD_ARG, "bad argument");
  if (n_values < 1 || n_values > 1000 || label_len > 255) return fail(EG_ERR_BAD_ARG, "n_values in 1..1000, label up to 255 bytes");
  Engine* e = nullptr;
  size_t item = 0;
  TRY(engine_create(c, eghost::build_sumsq_plan(n_values, std::string(label ? label : "", label_len), &item), pk, 0, &e));
  *out = new eg_proof_params{e, EG_PROOF_SUMSQ, item};
  (*out)->n_values = n_values;
  return EG_OK;
}
int eg_commit_equiv_params_create(eg_ctx* c, const uint8_t pk[32], const uint8_t blinding_base[32], const char* label, size_t label_len,
                                  eg_proof_params** out) { EG_LOCK(c);
  if (!c || !pk || !blinding_base || !out || (!label && label_len)) return fail(EG_ERR_BAD_ARG, "bad argument");
  if (label_len > 255) return fail(EG_ERR_BAD_ARG, "label up to 255 bytes");
  Engine* e = nullptr;
  TRY(engine_create(c, eghost::build_commit_equiv_plan(std::string(label ? label : "", label_len)), pk, 0, &e, blinding_base));
  *out = new eg_proof_params{e, EG_PROOF_COMMIT_EQUIV, eghost::COMMIT_EQUIV_ITEM};
  return EG_OK;
}
void eg_proof_params_destroy(eg_proof_params* p) { params_destroy(p); }
size_t eg_proof_item_size(const eg_proof_params* p) { return p ? p->item_size : 0; }
int eg_verify_proof_batch(eg_proof_params* p, size_t n, const uint8_t* items, uint32_t* status) { EG_LOCK_P(p);
  if (!p || (n && (!items || !status))) return fail(EG_ERR_BAD_ARG, "bad argument");
  return engine_verify_host(p->eng, n, items, status, nullptr);
}
int eg_verify_proof_batch_device(eg_proof_params* p, size_t n, const void* d_items, void* d_status, void* stream) { EG_LOCK_P(p);
  if (!p || (n && (!d_items || !d_status))) return fail(EG_ERR_BAD_ARG, "bad argument");
  HIPCHK(hipSetDevice(p->eng->ctx->device));
  return engine_verify_device(p->eng, n, d_items, d_status, (hipStream_t)stream);
}

// ---- host-only introspection (no GPU needed): the product's own RangeDecomposition and plan builders ----------------------------
int eg_range_decomposition(uint64_t upper_bound, char* buf, size_t cap) {
  if (upper_bound < 2 || !buf || cap == 0) return fail(EG_ERR_BAD_ARG, "upper_bound must be >= 2");   // range.rs:160
  const std::string t = eghost::optimal_range(upper_bound).to_string();
  if (t.size() + 1 > cap) return fail(EG_ERR_BAD_ARG, "buffer too small");
  memcpy(buf, t.c_str(), t.size() + 1);
  return EG_OK;
}
int eg_plan_describe(int kind, int n_options, uint64_t credits_or_bound, char* buf, size_t cap) {
  if (!buf || cap == 0) return fail(EG_ERR_BAD_ARG, "bad argument");
  eghost::Plan P;
  size_t item = 0;
  switch (kind) {
    case 0: P = eghost::build_choice_plan(n_options, true, choice_ring_group()); break;
    case 1: P = eghost::build_choice_plan(n_options, false, choice_ring_group()); break;
    case 2: P = eghost::build_qv_plan(n_options, credits_or_bound); break;
    case 3: P = eghost::build_zero_plan(); break;
    case 4: P = eghost::build_bool_plan(); break;
    case 5: P = eghost::build_range_plan(credits_or_bound, &item); break;
    case 6: P = eghost::build_sumsq_plan(n_options, "test", &item); break;
    case 7: P = eghost::build_commit_equiv_plan("test"); break;
    default: return fail(EG_ERR_BAD_ARG, "unknown plan kind");
  }
  size_t jobs = 0, insts = 0, var_terms = P.vterms.size(), table_terms = 0, derived = 0;
  size_t combs = 0, deferred = 0, plain_encodes = 0, inversion_groups = 0, derive_terms = P.dterms.size();
  size_t jobs_table1 = 0, chains = 0, chain_extra_terms = 0, loose_table_terms = 0, direct_terms = 0;
  std::string per_stage;
  for (auto& st : P.stages) {
    jobs += st.jobs.size(); insts += st.insts.size();
    per_stage += (per_stage.empty() ? "" : ",") + std::to_string(st.jobs.size());
    for (auto& j : st.jobs) {
      combs += (j.g.kind != egplan::SRC_NONE) + (j.k.kind != egplan::SRC_NONE) + (j.h != 0);
      if (j.defer) ++deferred; else ++plain_encodes;
      switch (job_family(j, P.vterms)) {
        case FAM_TABLE1: ++jobs_table1; break;
        case FAM_TABLEN:
          for (int t0 = 0; t0 < (int)j.term_count; t0 += EG_MULTI_GROUP) {
            ++chains;
            chain_extra_terms += std::min<int>(EG_MULTI_GROUP, j.term_count - t0) - 1;
          }
          break;
        case FAM_DIRECT1: ++direct_terms; break;
        case FAM_GENERIC:
          for (unsigned t = 0; t < j.term_count; ++t)
            if (P.vterms[j.term_first + t].base == 0xffff) ++direct_terms; else ++loose_table_terms;
          break;
        default: break;
      }
    }
    inversion_groups += (st.deferred.size() + 31) / 32;
  }
  for (auto& t : P.vterms) table_terms += t.base != 0xffff;
  for (auto& l : P.derive_levels) derived += l.size();
  char tmp[2048];
  snprintf(tmp, sizeof tmp,
           "{\"stride\": %zu, \"wire_points\": %zu, \"wire_scalars\": %zu, \"derived_points\": %zu, \"derive_terms\": %zu, \"bases\": %zu, "
           "\"stages\": %zu, \"jobs\": %zu, \"jobs_per_stage\": [%s], \"var_terms\": %zu, \"table_terms\": %zu, "
           "\"combs\": %zu, \"deferred\": %zu, \"plain_encodes\": %zu, \"inversion_groups\": %zu, "
           "\"single_table_jobs\": %zu, \"chains\": %zu, \"chain_extra_terms\": %zu, \"loose_table_terms\": %zu, \"direct_terms\": %zu, "
           "\"sum_tables\": %zu, \"sum_table_members\": %zu, "
           "\"hash_programs\": %zu, \"prefixes\": %d, \"flags\": %d, \"rules\": %zu, \"tally_slots\": %zu, "
           "\"pt_slots\": %d, \"cmp_slots\": %d, \"chal_slots\": %d, \"state_slots\": %d, \"tables\": %zu, \"teeth\": %d, "
           "\"ring_group\": %d, \"table_groups\": %zu}",
           P.stride, P.pt_items.size(), P.sc_items.size(), derived, derive_terms, P.base_slots.size(), P.stages.size(), jobs, per_stage.c_str(),
           var_terms, table_terms, combs, deferred, plain_encodes, inversion_groups, jobs_table1, chains, chain_extra_terms,
           loose_table_terms, direct_terms, P.sum_bases.size(), P.sum_members.size(), insts, P.n_prefixes, P.n_flag_slots, P.rules.size(),
           P.tally_slots.size(), P.n_pt_slots, P.n_cmp_slots, P.n_chal_slots, P.n_state_slots, (size_t)P.n_tables(), eghost::plan_teeth(P),
           P.ring_group, P.group_stage.size());
  if (strlen(tmp) + 1 > cap) return fail(EG_ERR_BAD_ARG, "buffer too small");
  memcpy(buf, tmp, strlen(tmp) + 1);
  return EG_OK;
}

// ---- wire ingest: serde's human-readable (JSON, base64url) layout -> packed ballots; host only (wire_json.hpp) --------------------
static int pack_json_common(const char* json, size_t json_len, int threads, size_t max_objects, size_t* n_objects,
                            std::vector<std::pair<size_t, size_t>>& spans) {
  if (!json_len) { if (n_objects) *n_objects = 0; return EG_OK; }
  if (!egwire::split_objects_parallel(json, json_len, threads, spans))
    return fail(EG_ERR_BAD_ARG, "the text is neither a JSON array of objects nor a sequence of JSON objects");
  if (n_objects) *n_objects = spans.size();
  if (spans.size() > max_objects) return fail(EG_ERR_BAD_ARG, "more objects in the text than max_objects (*n_objects says how many)");
  return EG_OK;
}
int eg_choice_pack_json(int n_options, int single, const char* json, size_t json_len, int threads, size_t max_objects,
                        uint8_t* packed, uint32_t* status, size_t* n_objects) {
  if (n_options < 1 || n_options > 4000 || (json_len && !json) || (max_objects && (!packed || !status)))
    return fail(EG_ERR_BAD_ARG, "bad argument");
  std::vector<std::pair<size_t, size_t>> spans;
  TRY(pack_json_common(json, json_len, threads, max_objects, n_objects, spans));
  const size_t stride = eghost::choice_ballot_size(n_options, single != 0);
  egwire::pack_parallel(json, spans, stride, threads, packed, status,
                        [&](egwire::Cursor& c, uint8_t* dst) { return egwire::pack_choice(c, n_options, single != 0, dst); });
  return EG_OK;
}
int eg_qv_pack_json(int n_options, uint64_t credits, const char* json, size_t json_len, int threads, size_t max_objects,
                    uint8_t* packed, uint32_t* status, size_t* n_objects) {
  if (n_options < 1 || n_options > 256 || credits < 1 || credits > 100000 || (json_len && !json) || (max_objects && (!packed || !status)))
    return fail(EG_ERR_BAD_ARG, "bad argument");
  std::vector<std::pair<size_t, size_t>> spans;
  TRY(pack_json_common(json, json_len, threads, max_objects, n_objects, spans));
  const eghost::QvShape sh = eghost::qv_shape(n_options, credits);
  const egwire::RangeShape vote{sh.vote_range.rings.size(), (size_t)sh.vote_range.rings_size()};
  const egwire::RangeShape credit{sh.credit_range.rings.size(), (size_t)sh.credit_range.rings_size()};
  egwire::pack_parallel(json, spans, sh.ballot_size, threads, packed, status, [&](egwire::Cursor& c, uint8_t* dst) {
    return egwire::pack_qv(c, n_options, vote, credit, sh.ballot_size, dst);
  });
  return EG_OK;
}
// JSON text -> verdicts + tally in one call.  The text is cut into windows (egwire::split_next); a producer thread splits and packs
// them on a pool of `threads` host threads into a pinned ring of packed ballots, while this thread uploads the finished windows and
// enqueues their verification, two submissions in flight (verify_json_common below).  Objects that do not pack keep their pack verdict;
// their zeroed slots are verified like any other ballot (an all-zero ballot never verifies, so nothing of it reaches the tally) and the
// verdict is overwritten afterwards.
typedef std::function<void(const char*, const std::vector<std::pair<size_t, size_t>>&, int, uint8_t*, uint32_t*, egwire::WorkerPool*)> PackPieceFn;
// verdicts of the objects that deserialise but do not have the election's shape (egwire::resolve_*_objects): false = a GPU call failed
typedef std::function<bool(const char*, const std::vector<std::pair<size_t, size_t>>&, std::vector<uint32_t>&)> ReshapeFn;
// the two GPU services of the object path (wire_json.hpp): validity of 32-byte items, and the batch verifier on substitute ballots
static egwire::CheckItemsFn make_check_items(eg_ctx* c) {
  return [c](const std::string& kinds, const egwire::Bytes& data, std::vector<uint8_t>& ok) {
    egwire::Bytes pts, scs;
    for (size_t i = 0; i < kinds.size(); ++i) {
      egwire::Bytes& dst = kinds[i] == 'P' ? pts : scs;
      dst.insert(dst.end(), data.begin() + 32 * i, data.begin() + 32 * (i + 1));
    }
    std::vector<uint8_t> pok(pts.size() / 32), sok(scs.size() / 32), tmp(pts.size());
    if (!pok.empty() && eg_point_roundtrip_batch(c, pok.size(), pts.data(), tmp.data(), pok.data())) return false;
    if (!sok.empty() && eg_scalar_is_canonical_batch(c, sok.size(), scs.data(), sok.data())) return false;
    ok.resize(kinds.size());
    size_t pi = 0, si = 0;
    for (size_t i = 0; i < kinds.size(); ++i) ok[i] = kinds[i] == 'P' ? pok[pi++] : sok[si++];
    return true;
  };
}
static int engine_verify_host(Engine* e, size_t n, const uint8_t* ballots, uint32_t* status, uint8_t* tally_out, bool small);
static egwire::VerifyPackedFn make_verify_packed(Engine* e) {
  return [e](size_t n, const egwire::Bytes& packed, std::vector<uint32_t>& status) {
    status.assign(n, 0);
    return engine_verify_host(e, n, packed.data(), status.data(), nullptr) == EG_OK;
  };
}
// ---- the JSON text in PIECES: eg_verify_{choice,qv}_json_begin[_multi] / eg_verify_json_feed / _feed_owned / _take / _end / _abort --------------
// (examples/voting.rs:195-198 emits ballots one at a time; src/serde.rs:19-80 is the layout.)  ONE worker thread per stream takes the
// pieces in order (stream_worker): it cuts a piece (egwire::StreamSplitter: values may straddle pieces), packs its complete ballots on
// the stream's pool of host threads into a pinned ring (stream_emit), and then PUMPS the GPU side without ever waiting for it
// (stream_pump) - retire the submissions that have landed, enqueue what has piled up (upload, verification on the two work sets, download
// of the verdicts).  The first submission goes once 2^14 ballots are packed (EG_JSON_FIRST_MIN; measured, profiles/r05_json_stream_probe.txt:
// 2^13 ... 2^14 ballots 0.91 of the HBM-resident rate, 2^15 0.90, 2^17 0.86 - waiting longer idles the GPU for longer than the small first
// launches cost), later ones when they are 1.5 x the one in flight, at most two in flight; the worker only waits for the GPU when the ring
// is full.  The one-shot entries (eg_verify_*_json[_multi]) are this pipeline fed with the whole text in place.  Between begin and end the
// params objects belong to the stream (other verify / tally calls on them are refused).
// SEVERAL GPUs (round 6; VERDICT r5 task 4a: the parser delivers 10 M ballots/s, one GPU takes 6): a stream has one LANE per params object -
// its own pinned ring, device staging, control streams and submissions in flight - and ONE splitter, pool and worker; every packed window
// goes to the lane with the fewest ballots waiting or in flight (a faster GPU, or one that started earlier, simply gets more windows), the
// verdicts are kept by object index (text order), and every params object tallies the windows it verified.
struct eg_json_stream {
  struct Region { size_t first, off, m; bool submitted; };
  struct Group { size_t n_regions, first, off, m; hipEvent_t uploaded, done; };
  struct Lane {
    Engine* e = nullptr;
    size_t cap = 0, first_min = 0, n_submitted = 0, pending = 0;   // pending: ballots in regions that have not been retired yet
    int n_ctl = 1;
    bool set_aside = false;
    std::deque<Region> regions;          // in text order; the front is the oldest one not yet retired
    std::deque<Group> groups;            // submissions in flight, oldest first
  };
  std::vector<Lane> lanes;               // one per params object; lanes[0]'s engine also resolves the ballots of another shape
  std::vector<eg_ctx*> ctxs;             // the lanes' contexts, each once, in address order: locked together (LockAll)
  Engine* e = nullptr;                   // = lanes[0].e
  int threads = 1, ns = 0;
  PackPieceFn pack_piece;
  ReshapeFn reshape;
  std::unique_ptr<egwire::WorkerPool> pool;
  std::unique_ptr<egwire::StreamSplitter> split;
  size_t stride = 0, growth = 150, emitted = 0;
  std::vector<uint32_t> verdicts;      // by object: its pack verdict until (if it packed) the GPU's verdict lands
  std::vector<uint32_t> pack_tmp;
  std::vector<std::string> odd_text;   // objects of another shape than the election's: resolved at the end (the object path needs the GPU to itself)
  std::vector<size_t> odd_at;
  size_t taken = 0;
  bool flushed = false, trace = false;
  bool one_shot = false;               // opened by eg_verify_*_json for the length of that call: other calls on the params objects wait for it
  size_t max_objects = (size_t)-1;     // one-shot: the room in the caller's status buffer; a text with more objects fails at once (stream_emit)
  size_t odd_bytes = 0, odd_max = (size_t)256 << 20;     // text of the ballots of another shape kept for the object path, and its bound (EG_JSON_ODD_MAX_MB)
  std::atomic<int> failed{EG_OK};      // set once (stream_fail), after err has been written
  std::string err;
  // Front end: the caller's pieces reach the worker thread through a short queue.  Pieces below `direct_min` are copied into blocks of
  // `block_bytes` (the caller's thread pays one memcpy and returns; cutting, packing and GPU submission happen on the worker thread, in
  // parallel with the caller producing the next piece); larger pieces are handed over in place and feed waits until the worker is through
  // with them.  Everything above (lanes, verdicts, splitter) is touched by the worker thread only, under the contexts' locks, until the
  // worker has been joined (end / abort) - take() takes those locks too.
  struct Item { std::vector<char> own; const char* ptr = nullptr; size_t len = 0; uint64_t id = 0; bool finish = false;
                eg_json_release_fn release = nullptr; void* user = nullptr; };      // release: a block handed over by eg_verify_json_feed_owned
  std::thread worker;
  std::mutex qmu;
  std::condition_variable q_push, q_pop;
  std::deque<Item> queue;
  std::vector<std::vector<char>> spare;    // emptied blocks
  std::vector<char> acc;                   // the block being filled by feed
  uint64_t next_id = 1, consumed_id = 0;
  size_t queued_bytes = 0;                 // text waiting in the queue (copied blocks and handed-over ones): at most ~64 MB, then feed waits
  bool stop = false, worker_joined = false;
  std::atomic<size_t> objects{0};          // complete objects cut so far (by the worker)
  size_t block_bytes = (size_t)16 << 20, direct_min = (size_t)8 << 20;
  // handed-over blocks joined per piece, and the text that may wait in the queue (8 / 32 / 64 MB pieces measured the same within the
  // +-4 % run-to-run noise of the stream: gpurun_out/json_owned_join_ab.txt, round 6)
  size_t join_bytes = (size_t)16 << 20, queue_bytes = (size_t)64 << 20;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();      // EG_JSON_TRACE: the timeline on stderr, ms since begin
  double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};
// every context of a stream's lanes, locked together in address order (one context: exactly the lock every entry point takes); the calling
// thread's current device, which the work on the lanes changes, is put back when the locks go
struct LockAll {
  KeepDevice keep;
  std::vector<std::unique_lock<std::recursive_mutex>> held;
  explicit LockAll(const std::vector<eg_ctx*>& ctxs) { for (eg_ctx* c : ctxs) held.emplace_back(c->mu); }
};
static bool stream_is_one_shot(const eg_json_stream* S) { return S->one_shot; }
static int stream_fail(eg_json_stream* S, int code, const std::string& msg) {
  if (!S->failed.load(std::memory_order_acquire)) { S->err = msg; S->failed.store(code, std::memory_order_release); }
  return fail(S->failed.load(), S->err);
}
typedef eg_json_stream::Lane StreamLane;
static void stream_retire_oldest(eg_json_stream* S, StreamLane& L) {     // the lane's oldest submission has landed: its verdicts, its part of the ring
  Engine* e = L.e;
  const eg_json_stream::Group g = L.groups.front();
  L.groups.pop_front();
  for (size_t k = 0; k < g.n_regions; ++k) {
    const eg_json_stream::Region r = L.regions.front();
    L.regions.pop_front();
    L.pending -= r.m;
    for (size_t i = 0; i < r.m; ++i)
      if (S->verdicts[r.first + i] == EG_ST_OK) S->verdicts[r.first + i] = e->json_status_ring[r.off + i];
  }
  (void)hipEventDestroy(g.uploaded); (void)hipEventDestroy(g.done);
  if (S->trace) fprintf(stderr, "[json stream] %8.2f ms  landed    %zu ballots from %zu (lane %d)\n", S->ms(), g.m, g.first, (int)(&L - S->lanes.data()));
}
// objects whose verdicts are final as far as the GPUs are concerned: everything before the oldest region any lane still holds
static size_t stream_landed(const eg_json_stream* S) {
  size_t upto = S->emitted;
  for (const StreamLane& L : S->lanes)
    if (!L.regions.empty()) upto = std::min(upto, L.regions.front().first);
  return upto;
}
// enqueue what has piled up on a lane, if it is time (or `force`: the ring is full, or the text has ended); never waits for the GPU
static int stream_pump(eg_json_stream* S, StreamLane& L, bool force) {
  Engine* e = L.e;
  if (hipSetDevice(e->ctx->device) != hipSuccess) return stream_fail(S, EG_ERR_HIP, "hipSetDevice");
  for (;;) {
    while (!L.groups.empty() && hipEventQuery(L.groups.front().done) == hipSuccess) stream_retire_oldest(S, L);
    (void)hipGetLastError();                           // a submission still running reads as hipErrorNotReady: not an error to keep
    if (L.groups.size() >= 2) return EG_OK;
    eg_json_stream::Group g{0, 0, 0, 0, nullptr, nullptr};
    for (auto& r : L.regions) {                        // the run of packed windows behind the submitted ones, contiguous in the ring
      if (r.submitted) continue;
      if (g.n_regions && r.off != g.off + g.m) break;
      if (!g.n_regions) { g.first = r.first; g.off = r.off; }
      ++g.n_regions; g.m += r.m;
    }
    if (!g.n_regions) return EG_OK;
    bool go = force;
    if (!go && L.groups.empty()) go = L.n_submitted ? true : g.m >= L.first_min;       // an idle GPU takes whatever there is - except the very first time
    if (!go && L.groups.size() == 1) go = g.m * 100 >= L.groups.back().m * S->growth && g.m >= std::min(L.first_min, L.cap / 8);
    if (!go) return EG_OK;
    hipStream_t ctl = e->json_ctl[L.n_submitted % (size_t)L.n_ctl];
    const char* what = "window upload: ";
    hipError_t he = hipEventCreateWithFlags(&g.uploaded, hipEventDisableTiming);
    if (he == hipSuccess) he = hipEventCreateWithFlags(&g.done, hipEventDisableTiming | hipEventBlockingSync);
    if (he == hipSuccess) he = hipMemcpyAsync(e->d_wire + g.off * S->stride, e->json_ring + g.off * S->stride, g.m * S->stride, hipMemcpyHostToDevice, e->copy_stream);
    if (he == hipSuccess) he = hipEventRecord(g.uploaded, e->copy_stream);
    if (he == hipSuccess) he = hipStreamWaitEvent(ctl, g.uploaded, 0);
    int rc = EG_OK;
    if (he == hipSuccess) {
      rc = engine_verify_device(e, g.m, e->d_wire + g.off * S->stride, e->d_status + g.off, ctl, VD_FORCE_SETS | VD_KEEP_SET_TALLY);
      what = "verdict download: ";
      if (rc == EG_OK) he = hipMemcpyAsync(e->json_status_ring + g.off, e->d_status + g.off, g.m * sizeof(u32), hipMemcpyDeviceToHost, ctl);
      if (rc == EG_OK && he == hipSuccess) he = hipEventRecord(g.done, ctl);
    }
    if (he != hipSuccess) rc = fail(EG_ERR_HIP, std::string(what) + hipGetErrorString(he));
    if (rc) {
      if (g.uploaded) (void)hipEventDestroy(g.uploaded);
      if (g.done) (void)hipEventDestroy(g.done);
      return stream_fail(S, rc, g_err);
    }
    size_t k = 0;
    for (auto& r : L.regions) { if (r.submitted) continue; if (k++ == g.n_regions) break; r.submitted = true; }
    L.groups.push_back(g);
    ++L.n_submitted;
    if (S->trace) fprintf(stderr, "[json stream] %8.2f ms  submitted %zu windows, %zu ballots from %zu (lane %d, %zu in flight)\n", S->ms(), g.n_regions, g.m, g.first, (int)(&L - S->lanes.data()), L.groups.size());
  }
}
static int stream_pump_all(eg_json_stream* S, bool force) {
  for (StreamLane& L : S->lanes) TRY(stream_pump(S, L, force));
  return EG_OK;
}
// room for m packed ballots in a lane's ring (behind its newest region, or from the start again once the oldest regions there have been
// retired); waits for the GPU only when there is none
static int stream_place(eg_json_stream* S, StreamLane& L, size_t m, size_t* off) {
  for (;;) {
    if (L.regions.empty()) { *off = 0; return EG_OK; }
    const size_t head = L.regions.back().off + L.regions.back().m, tail = L.regions.front().off;
    if (head > tail) {                            // the occupied part does not wrap
      if (head + m <= L.cap) { *off = head; return EG_OK; }
      if (m <= tail) { *off = 0; return EG_OK; }
    } else if (head + m <= tail) { *off = head; return EG_OK; }
    if (L.groups.empty()) {
      TRY(stream_pump(S, L, true));               // the ring is full of packed ballots nobody has submitted yet
      if (L.groups.empty()) return stream_fail(S, EG_ERR_NOMEM, "a window of ballots does not fit the staging ring");
    }
    (void)hipSetDevice(L.e->ctx->device);
    const hipError_t he = hipEventSynchronize(L.groups.front().done);
    if (he != hipSuccess) return stream_fail(S, EG_ERR_HIP, std::string("window: ") + hipGetErrorString(he));
    stream_retire_oldest(S, L);
  }
}
// the complete values of one window of the text: pack them into a lane's ring, remember the ones that need the object path, pump the GPUs
static bool stream_emit(eg_json_stream* S, const char* base, const std::vector<std::pair<size_t, size_t>>& spans, size_t first) {
  if (first + spans.size() > S->max_objects) {
    stream_fail(S, EG_ERR_BAD_ARG, "more objects in the text than max_objects");
    return false;
  }
  // the lane with the least work waiting or in flight whose ring has room without waiting; if none has, the least loaded one (it waits)
  StreamLane* best = nullptr;
  for (StreamLane& L : S->lanes)
    if (L.pending + spans.size() <= L.cap && (!best || L.pending < best->pending)) best = &L;
  if (!best)
    for (StreamLane& L : S->lanes)
      if (!best || L.pending < best->pending) best = &L;
  StreamLane& L = *best;
  Engine* e = L.e;
  size_t off = 0;
  if (stream_place(S, L, spans.size(), &off)) return false;
  S->pack_tmp.resize(spans.size());
  S->pack_piece(base, spans, S->threads, e->json_ring + off * S->stride, S->pack_tmp.data(), S->pool.get());
  if (S->verdicts.size() < first + spans.size()) S->verdicts.resize(first + spans.size());
  for (size_t i = 0; i < spans.size(); ++i) {
    S->verdicts[first + i] = S->pack_tmp[i];
    if (S->pack_tmp[i] == EG_PACK_RESHAPE) {
      // a ballot of another shape than the election's keeps its TEXT until the end (the object path needs the GPU to itself): bounded, so
      // that a text made of such objects cannot make the streaming entry buffer its whole input in host memory
      S->odd_bytes += spans[i].second;
      if (S->odd_bytes > S->odd_max) {
        stream_fail(S, EG_ERR_NOMEM, "the ballots whose shape is not the election's exceed " + std::to_string(S->odd_max >> 20) +
                                         " MB of text (EG_JSON_ODD_MAX_MB): verify such a text through the object path in smaller pieces");
        return false;
      }
      S->odd_text.emplace_back(base + spans[i].first, spans[i].second); S->odd_at.push_back(first + i);
    }
  }
  L.regions.push_back({first, off, spans.size(), false});
  L.pending += spans.size();
  S->emitted = first + spans.size();
  return stream_pump_all(S, false) == EG_OK;
}
static void stream_release(eg_json_stream* S, bool keep_partial_tally) {      // the engines go back to their owners; the stream is deleted
  for (StreamLane& L : S->lanes) {
    Engine* e = L.e;
    (void)hipSetDevice(e->ctx->device);
    (void)hipDeviceSynchronize();                         // nothing may still read the ring or the work sets
    for (auto& g : L.groups) { if (g.uploaded) (void)hipEventDestroy(g.uploaded); if (g.done) (void)hipEventDestroy(g.done); }
    L.groups.clear();
    hipStream_t s = e->ctx->stream;
    if (S->ns && e->n_sets == 2) {
      if (keep_partial_tally) hipLaunchKernelGGL(k_tally_add_points, dim3(blocks_of((size_t)S->ns)), dim3(NT), 0, s, e->set[1].tally, S->ns, e->set[0].tally);
      hipLaunchKernelGGL(k_tally_init, dim3(blocks_of((size_t)S->ns)), dim3(NT), 0, s, e->set[1].tally, S->ns);
    }
    if (L.set_aside && S->ns) {
      // a finished stream: running tally = what it was + the stream's ballots on this lane; an aborted or failed one: what it was
      if (keep_partial_tally) hipLaunchKernelGGL(k_tally_add_points, dim3(blocks_of((size_t)S->ns)), dim3(NT), 0, s, e->tally_saved2, S->ns, e->tally);
      else (void)hipMemcpyAsync(e->tally, e->tally_saved2, (size_t)S->ns * PT_WORDS * sizeof(u32), hipMemcpyDeviceToDevice, s);
    }
    (void)hipStreamSynchronize(s);
    e->stream_open = nullptr;
  }
  delete S;
}
static void stream_worker(eg_json_stream* S);
// size_hint: bytes of text to come if the caller knows (the one-shot entry does: a short text gets a short ring), else 0.  Called with every
// engine's context locked (LockAll) and no stream open on any of them.
static int stream_begin(const std::vector<Engine*>& engines, int threads, PackPieceFn pack_piece, ReshapeFn reshape, size_t size_hint, eg_json_stream** out) {
  if (!out || engines.empty()) return fail(EG_ERR_BAD_ARG, "bad argument");
  *out = nullptr;
  for (Engine* e : engines)
    if (e->stream_open) return fail(EG_ERR_BAD_ARG, "a JSON stream is already open on this params object");
  std::unique_ptr<eg_json_stream> S(new eg_json_stream());
  Engine* e0 = engines[0];
  S->e = e0; S->threads = std::max(threads, 1); S->pack_piece = std::move(pack_piece); S->reshape = std::move(reshape);
  S->stride = e0->plan.stride; S->ns = (int)e0->plan.tally_slots.size();
  S->growth = e0->knobs.json_growth; S->trace = e0->knobs.json_trace;
  S->odd_max = e0->knobs.json_odd_max_mb << 20;
  const size_t n_lanes = engines.size();
  S->lanes.resize(n_lanes);
  // if anything below fails, the lanes that were already set up get their running tallies back
  size_t lanes_ready = 0;
  ScopeExit undo{[&]() {
    if (!S) return;                              // released to the caller: success
    for (size_t k = 0; k < lanes_ready; ++k) {
      Engine* e = S->lanes[k].e;
      if (!S->lanes[k].set_aside || !S->ns) continue;
      (void)hipSetDevice(e->ctx->device);
      (void)hipMemcpyAsync(e->tally, e->tally_saved2, (size_t)S->ns * PT_WORDS * sizeof(u32), hipMemcpyDeviceToDevice, e->ctx->stream);
      (void)hipStreamSynchronize(e->ctx->stream);
    }
  }};
  for (size_t k = 0; k < n_lanes; ++k) {
    Engine* e = engines[k];
    StreamLane& L = S->lanes[k];
    L.e = e;
    HIPCHK(hipSetDevice(e->ctx->device));
    hipStream_t s = e->ctx->stream;
    HIPCHK(hipDeviceSynchronize());
    // one GiB of pinned staging for one GPU; several GPUs share that budget (at least 128 MiB each)
    const size_t ring_max = std::max((e->knobs.json_ring_kb ? e->knobs.json_ring_kb << 10 : (size_t)1 << 30) / n_lanes,
                                     e->knobs.json_ring_kb ? (size_t)0 : (size_t)128 << 20);
    const size_t hint = size_hint ? size_hint / n_lanes : 0;
    const size_t ring_bytes = std::max(hint ? std::min(hint / 4 * 3 + S->stride, ring_max) : ring_max, 64 * S->stride);
    L.cap = ring_bytes / S->stride;
    L.first_min = std::min<size_t>(e->knobs.json_first_min ? e->knobs.json_first_min : (size_t)1 << 14, L.cap / 4);
    if (L.cap * S->stride > e->json_ring_bytes || L.cap > e->json_ring_ballots) {
      if (e->json_ring) (void)hipHostFree(e->json_ring);
      if (e->json_status_ring) (void)hipHostFree(e->json_status_ring);
      e->json_ring = nullptr; e->json_status_ring = nullptr; e->json_ring_bytes = 0; e->json_ring_ballots = 0;
      if (hipHostMalloc((void**)&e->json_ring, L.cap * S->stride, hipHostMallocPortable) != hipSuccess ||
          hipHostMalloc((void**)&e->json_status_ring, L.cap * sizeof(u32), hipHostMallocPortable) != hipSuccess) {
        (void)hipGetLastError();
        return fail(EG_ERR_NOMEM, "pinned staging allocation failed");
      }
      e->json_ring_bytes = L.cap * S->stride; e->json_ring_ballots = L.cap;
    } else L.cap = std::min(L.cap, e->json_ring_ballots);
    TRY(engine_stage_reserve(e, L.cap));
    if (!e->copy_stream) HIPCHK(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
    L.n_ctl = e->n_sets == 2 ? 2 : 1;
    for (int c = 0; c < L.n_ctl; ++c)
      if (!e->json_ctl[c]) HIPCHK(hipStreamCreateWithFlags(&e->json_ctl[c], hipStreamNonBlocking));
    {
      const size_t per_set = (L.cap + e->n_sets - 1) / e->n_sets + NT;
      const int rr = engine_reserve(e, (u32)std::min<size_t>(per_set, e->max_cap));
      if (rr != EG_OK && rr != EG_ERR_NOMEM) return rr;
    }
    if (S->ns) {        // the stream's own tally is reported at the end; the running tally keeps accumulating (eg_hip.h)
      HIPCHK(hipMemcpyAsync(e->tally_saved2, e->tally, (size_t)S->ns * PT_WORDS * sizeof(u32), hipMemcpyDeviceToDevice, s));
      hipLaunchKernelGGL(k_tally_init, dim3(blocks_of((size_t)S->ns)), dim3(NT), 0, s, e->tally, S->ns);
      L.set_aside = true;
    }
    lanes_ready = k + 1;
    HIPCHK(hipStreamSynchronize(s));
    if (std::find(S->ctxs.begin(), S->ctxs.end(), e->ctx) == S->ctxs.end()) S->ctxs.push_back(e->ctx);
  }
  std::sort(S->ctxs.begin(), S->ctxs.end(), std::less<eg_ctx*>());
  S->pool.reset(new egwire::WorkerPool(S->threads));
  eg_json_stream* raw = S.get();
  const size_t window = e0->knobs.json_window_kb ? e0->knobs.json_window_kb << 10 : (size_t)32 << 20;
  size_t min_cap = S->lanes[0].cap;
  for (const StreamLane& L : S->lanes) min_cap = std::min(min_cap, L.cap);
  S->split.reset(new egwire::StreamSplitter(S->threads, S->pool.get(),
                                            [raw](const char* base, const std::vector<std::pair<size_t, size_t>>& spans, size_t first) {
                                              return stream_emit(raw, base, spans, first);
                                            },
                                            window, std::max<size_t>(1, min_cap / 8)));
  for (Engine* e : engines) e->stream_open = raw;
  if (S->trace) fprintf(stderr, "[json stream] %8.2f ms  begun (%zu lane(s), rings of %zu ballots, first submission from %zu)\n", S->ms(), n_lanes, S->lanes[0].cap, S->lanes[0].first_min);
  S->worker = std::thread(stream_worker, raw);
  *out = S.release();
  return EG_OK;
}
// the worker thread of a stream: pieces in order through the splitter (-> stream_emit -> rings, GPUs), each under the contexts' locks
static void stream_worker(eg_json_stream* S) {
  std::vector<char> joined;                 // small handed-over blocks that were waiting together, copied into one piece (below)
  for (;;) {
    eg_json_stream::Item it;
    std::vector<eg_json_stream::Item> more;      // the handed-over blocks behind `it` that are processed with it
    {
      std::unique_lock<std::mutex> lk(S->qmu);
      S->q_push.wait(lk, [&]() { return S->stop || !S->queue.empty(); });
      if (S->stop) return;
      it = std::move(S->queue.front());
      S->queue.pop_front();
      // Small blocks handed over by eg_verify_json_feed_owned are cheap to take one by one only when they arrive slowly: every piece costs
      // a hand-over, a window of the splitter, two dispatches on the pool (a ballot straddles almost every boundary) and a look at the
      // GPU - 1 MB pieces at the rate of the verifier are 1 400 of those in 160 ms (measured: 0.48 of the resident rate).  Blocks that are
      // WAITING TOGETHER are therefore joined into one piece of up to 16 MB, copied by the pool's threads (not by the caller's, and not one
      // after the other), and given back at once: 0.85-0.91.
      if (it.release && !it.finish && it.len < S->direct_min) {
        size_t total = it.len;
        while (!S->queue.empty() && S->queue.front().release && !S->queue.front().finish && S->queue.front().len < S->direct_min &&
               total + S->queue.front().len <= S->join_bytes) {
          total += S->queue.front().len;
          more.push_back(std::move(S->queue.front()));
          S->queue.pop_front();
        }
      }
    }
    const char* text = it.ptr ? it.ptr : it.own.data();
    size_t len = it.len;
    for (auto& m : more) len += m.len;
    // nothing thrown on this thread may escape it (std::terminate): out of host memory while joining blocks, growing the verdict vector or
    // keeping the text of odd ballots becomes the stream's error, reported by the next feed / take / end like every other
    try {
      if (!more.empty()) {
        std::vector<const eg_json_stream::Item*> parts{&it};
        for (auto& m : more) parts.push_back(&m);
        if (joined.size() < len) joined.resize(len);
        std::vector<size_t> at(parts.size(), 0);
        for (size_t k = 1; k < parts.size(); ++k) at[k] = at[k - 1] + parts[k - 1]->len;
        S->pool->run(parts.size(), 1, [&](size_t lo, size_t hi) { for (size_t k = lo; k < hi; ++k) if (parts[k]->len) memcpy(joined.data() + at[k], parts[k]->ptr, parts[k]->len); });
        text = joined.data();
        if (it.release) { it.release(it.user, it.ptr, it.len); it.release = nullptr; }     // copied: the blocks go back before they are parsed
        for (auto& m : more) { m.release(m.user, m.ptr, m.len); m.release = nullptr; }
      }
      if (!it.finish && !S->failed.load(std::memory_order_acquire)) {
        LockAll lk(S->ctxs);
        if (!S->split->feed(text, len)) {
          if (!S->failed.load()) stream_fail(S, EG_ERR_BAD_ARG, S->split->error().empty() ? std::string("the piece could not be packed") : S->split->error());
        } else (void)stream_pump_all(S, false);
        S->objects.store(S->split->count(), std::memory_order_release);
      }
    } catch (const std::bad_alloc&) { stream_fail(S, EG_ERR_NOMEM, "out of host memory in the stream's worker");
    } catch (const std::exception& ex) { stream_fail(S, EG_ERR_HIP, std::string("exception in the stream's worker: ") + ex.what());
    } catch (...) { stream_fail(S, EG_ERR_HIP, "unknown exception in the stream's worker"); }
    for (auto& m : more)                           // (only after an exception above: blocks that were not given back yet)
      if (m.release) { m.release(m.user, m.ptr, m.len); m.release = nullptr; }
    {
      std::lock_guard<std::mutex> lk(S->qmu);
      S->consumed_id = more.empty() ? it.id : more.back().id;
      S->queued_bytes -= std::min(S->queued_bytes, len);
      if (!it.own.empty() || it.own.capacity()) { it.own.clear(); S->spare.push_back(std::move(it.own)); }
    }
    S->q_pop.notify_all();
    if (it.release) it.release(it.user, it.ptr, it.len);      // the caller's block goes back: nothing of it is referenced any more
    if (it.finish) return;
  }
}
// hands an item to the worker (at most ~64 MB of text wait in the queue); wait = until the worker is through with it
static void stream_enqueue(eg_json_stream* S, std::unique_lock<std::mutex>& lk, eg_json_stream::Item&& it, bool wait) {
  S->q_pop.wait(lk, [&]() { return S->queue.empty() || S->queued_bytes < S->queue_bytes; });
  const uint64_t id = it.id = S->next_id++;
  S->queued_bytes += it.len;
  S->queue.push_back(std::move(it));
  S->q_push.notify_one();
  if (wait) S->q_pop.wait(lk, [&]() { return S->consumed_id >= id; });
}
static void stream_flush_acc(eg_json_stream* S, std::unique_lock<std::mutex>& lk) {
  if (S->acc.empty()) return;
  eg_json_stream::Item it;
  it.len = S->acc.size();
  it.own = std::move(S->acc);
  S->acc = std::vector<char>();
  if (!S->spare.empty()) { S->acc = std::move(S->spare.back()); S->spare.pop_back(); }
  stream_enqueue(S, lk, std::move(it), false);
}
static void stream_join_worker(eg_json_stream* S, bool finish) {      // never called with a context's lock held: the worker takes them per piece
  if (S->worker_joined) return;
  {
    std::unique_lock<std::mutex> lk(S->qmu);
    if (finish) {
      stream_flush_acc(S, lk);
      eg_json_stream::Item fin;
      fin.finish = true;
      stream_enqueue(S, lk, std::move(fin), false);
    } else {
      S->stop = true;
      S->q_push.notify_all();
    }
  }
  if (S->worker.joinable()) S->worker.join();
  S->worker_joined = true;
  for (auto& it : S->queue)                 // an aborted stream: handed-over blocks the worker never got to go back to their owner
    if (it.release) it.release(it.user, it.ptr, it.len);
  S->queue.clear();
}
int eg_verify_json_feed(eg_json_stream* S, const char* text, size_t len, size_t* n_objects) {
  if (!S || (len && !text)) return fail(EG_ERR_BAD_ARG, "bad argument");
  {
    std::unique_lock<std::mutex> lk(S->qmu);
    if (S->failed.load(std::memory_order_acquire)) return fail(S->failed.load(), S->err);
    if (S->flushed || S->worker_joined) return fail(EG_ERR_BAD_ARG, "the stream has been ended");
    if (len >= S->direct_min) {                    // a large piece: in place, and feed returns when the worker is through with it
      stream_flush_acc(S, lk);
      eg_json_stream::Item it;
      it.ptr = text; it.len = len;
      stream_enqueue(S, lk, std::move(it), true);
    } else {
      while (len) {                                // small pieces: copied into the block that is being filled
        if (S->acc.capacity() < S->block_bytes) S->acc.reserve(S->block_bytes);
        const size_t take = std::min(len, S->block_bytes - S->acc.size());
        S->acc.insert(S->acc.end(), text, text + take);
        text += take; len -= take;
        if (S->acc.size() >= S->block_bytes) stream_flush_acc(S, lk);
      }
    }
    if (S->failed.load(std::memory_order_acquire)) return fail(S->failed.load(), S->err);
  }
  if (n_objects) *n_objects = S->objects.load(std::memory_order_acquire);
  return EG_OK;
}
// The next piece WITHOUT a copy and without waiting: the library reads the caller's block in place and calls release(user, text, len) -
// from the stream's worker thread, or from the thread that ends / aborts the stream - when nothing of it is referenced any more.
// (eg_verify_json_feed copies a small piece on the caller's thread: 1.5 GB of text in 1 MB pieces is 150 ms of memcpy, as long as the GPU
// needs for the million ballots in it - json_stream.pieces.1MB of the bench line sat at 0.83 of the resident rate for that reason.)
int eg_verify_json_feed_owned(eg_json_stream* S, const char* text, size_t len, eg_json_release_fn release, void* user, size_t* n_objects) {
  if (!S || !release || (len && !text)) return fail(EG_ERR_BAD_ARG, "bad argument");
  {
    std::unique_lock<std::mutex> lk(S->qmu);
    if (S->failed.load(std::memory_order_acquire)) return fail(S->failed.load(), S->err);
    if (S->flushed || S->worker_joined) return fail(EG_ERR_BAD_ARG, "the stream has been ended");
    stream_flush_acc(S, lk);                        // pieces copied earlier come first
    eg_json_stream::Item it;
    it.ptr = text; it.len = len; it.release = release; it.user = user;
    stream_enqueue(S, lk, std::move(it), false);    // from here on the block is the library's: release will be called, whatever happens
  }
  if (n_objects) *n_objects = S->objects.load(std::memory_order_acquire);
  return EG_OK;
}
// A ready-made release function for eg_verify_json_feed_owned: counts the blocks that came back in the size_t that `user` points to.  For
// bindings whose own callbacks are expensive - a Python (ctypes) callback takes the interpreter lock on the stream's worker thread, once per
// block, in competition with the thread that is feeding - and for tests that only want to know that every block was given back.
void eg_json_release_count(void* user, const char*, size_t) {
  if (user) __atomic_fetch_add(static_cast<size_t*>(user), (size_t)1, __ATOMIC_RELAXED);
}
// verdicts that are final so far, in order, from where the last take stopped: every ballot before the first one that is still on a GPU
// or waits for the object path (a ballot of another shape than the election's gets its verdict at the end)
static size_t stream_final_upto(const eg_json_stream* S) {
  size_t upto = S->flushed ? S->verdicts.size() : stream_landed(S);
  if (!S->flushed && !S->odd_at.empty()) upto = std::min(upto, S->odd_at.front());
  return upto;
}
int eg_verify_json_take(eg_json_stream* S, uint32_t* status, size_t cap, size_t* n_taken) {
  if (!S || !n_taken || (cap && !status)) return fail(EG_ERR_BAD_ARG, "bad argument");
  *n_taken = 0;
  if (S->failed.load(std::memory_order_acquire)) return fail(S->failed.load(), S->err);
  {   // pieces copied so far go to the worker now: a slow source gets its verdicts without waiting for a block to fill up
    std::unique_lock<std::mutex> lk(S->qmu);
    if (!S->flushed && !S->worker_joined) stream_flush_acc(S, lk);
  }
  LockAll lk(S->ctxs);                              // the worker holds them while it cuts and packs a piece
  if (!S->flushed)
    for (StreamLane& L : S->lanes) TRY(stream_pump(S, L, L.groups.empty()));     // an idle GPU takes what has been packed, however little
  const size_t upto = stream_final_upto(S);
  const size_t n = std::min(cap, upto > S->taken ? upto - S->taken : 0);
  if (n) memcpy(status, S->verdicts.data() + S->taken, n * sizeof(uint32_t));
  S->taken += n;
  *n_taken = n;
  return EG_OK;
}
int eg_verify_json_end(eg_json_stream* S, uint32_t* status, size_t cap, size_t* n_taken, size_t* n_objects, uint8_t* tally_out) {
  if (!S || (cap && !status)) return fail(EG_ERR_BAD_ARG, "bad argument");
  stream_join_worker(S, true);                      // every piece cut and packed; from here on this thread owns the stream
  LockAll lk(S->ctxs);
  if (S->trace) fprintf(stderr, "[json stream] %8.2f ms  every piece packed (%zu objects)\n", S->ms(), S->split->count());
  if (n_taken) *n_taken = 0;
  Engine* e = S->e;
  if (!S->flushed && !S->failed.load()) {
    if (!S->split->finish()) stream_fail(S, EG_ERR_BAD_ARG, S->split->error());
    for (;;) {                                     // every lane: submit what is left, wait for what is in flight, oldest first
      if (S->failed.load()) break;
      bool busy = false;
      for (StreamLane& L : S->lanes) {
        if (L.regions.empty() && L.groups.empty()) continue;
        busy = true;
        if (stream_pump(S, L, true)) break;
        if (L.groups.empty()) continue;
        (void)hipSetDevice(L.e->ctx->device);
        const hipError_t he = hipEventSynchronize(L.groups.front().done);
        if (he != hipSuccess) { stream_fail(S, EG_ERR_HIP, std::string("window: ") + hipGetErrorString(he)); break; }
        stream_retire_oldest(S, L);
      }
      if (!busy) break;
    }
    if (!S->failed.load())
      for (StreamLane& L : S->lanes) {
        Engine* le = L.e;
        (void)hipSetDevice(le->ctx->device);
        (void)hipDeviceSynchronize();
        hipStream_t s = le->ctx->stream;
        if (S->ns && le->n_sets == 2) {                           // the sets' shares of the tally, once
          hipLaunchKernelGGL(k_tally_add_points, dim3(blocks_of((size_t)S->ns)), dim3(NT), 0, s, le->set[1].tally, S->ns, le->set[0].tally);
          hipLaunchKernelGGL(k_tally_init, dim3(blocks_of((size_t)S->ns)), dim3(NT), 0, s, le->set[1].tally, S->ns);
          if (hipStreamSynchronize(s) != hipSuccess) stream_fail(S, EG_ERR_HIP, "tally merge failed");
        }
      }
    if (!S->failed.load() && !S->odd_at.empty()) {   // OptionsLenMismatch / LenMismatch territory: the object path, in the reference's order of checks
      std::string all;
      std::vector<std::pair<size_t, size_t>> spans;
      for (auto& t : S->odd_text) { spans.push_back({all.size(), t.size()}); all += t; all += '\n'; }
      std::vector<uint32_t> v;
      e->stream_open = nullptr;               // the object path verifies substitute ballots through the ordinary host entry of the first lane's engine
      const bool ok = S->reshape(all.data(), spans, v);
      e->stream_open = S;
      if (!ok) stream_fail(S, EG_ERR_HIP, g_err.empty() ? std::string("object path: a GPU call failed") : g_err);
      else for (size_t i = 0; i < S->odd_at.size(); ++i) S->verdicts[S->odd_at[i]] = v[i];
    }
    S->flushed = true;
  }
  if (S->failed.load()) {
    const int rc = S->failed.load();
    const std::string why = S->err;
    stream_release(S, false);
    return fail(rc, why);
  }
  const size_t left = S->verdicts.size() - S->taken;
  if (left > cap) {            // the stream stays open (and flushed): *n_taken says how much room the caller must come back with
    if (n_taken) *n_taken = left;
    return fail(EG_ERR_BAD_ARG, "status holds " + std::to_string(cap) + " verdicts, " + std::to_string(left) + " are left: call again with room for them (or eg_verify_json_abort)");
  }
  if (left) memcpy(status, S->verdicts.data() + S->taken, left * sizeof(uint32_t));
  if (n_taken) *n_taken = left;
  if (n_objects) *n_objects = S->verdicts.size();
  int rc = EG_OK;
  if (S->trace) fprintf(stderr, "[json stream] %8.2f ms  verdicts copied\n", S->ms());
  if (tally_out && S->ns) {       // the stream's own tally = the sum of its lanes' (every running tally gets its lane's share added below)
    const size_t bytes = (size_t)S->ns * 32;
    std::vector<uint8_t> part(bytes), ok(S->ns);
    for (size_t k = 0; k < S->lanes.size() && !rc; ++k) {
      (void)hipSetDevice(S->lanes[k].e->ctx->device);
      rc = engine_tally_encode(S->lanes[k].e, k == 0 ? tally_out : part.data());
      if (!rc && k) {
        rc = eg_point_add_batch(e->ctx, (size_t)S->ns, tally_out, part.data(), 0, tally_out, ok.data());
        if (!rc) for (uint8_t o : ok) if (!o) rc = fail(EG_ERR_HIP, "the tally of lane " + std::to_string(k) + " does not decode");
      }
    }
  }
  const std::string why = g_err;
  const bool trace = S->trace;
  const auto t0 = S->t0;
  stream_release(S, true);
  if (trace) fprintf(stderr, "[json stream] %8.2f ms  released\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  return rc ? fail(rc, why) : EG_OK;
}
void eg_verify_json_abort(eg_json_stream* S) {
  if (!S) return;
  stream_join_worker(S, false);
  const std::vector<eg_ctx*> ctxs = S->ctxs;      // (the stream is deleted under the locks)
  LockAll lk(ctxs);
  stream_release(S, false);
}
// Opens a stream over one or several params objects.  one_shot: for the length of an eg_verify_*_json[_multi] call, whose caller holds the
// engines' long_call_mu; an explicit begin takes them only while it opens the stream (so that it waits for a long call that is running on
// any of the objects, as every entry point does).
static int stream_open_on(const std::vector<Engine*>& engines, int threads, PackPieceFn pack_piece, ReshapeFn reshape, size_t size_hint, bool one_shot,
                          size_t max_objects, eg_json_stream** out) {
  std::vector<Engine*> order(engines);
  std::sort(order.begin(), order.end(), std::less<Engine*>());
  std::vector<std::unique_lock<std::mutex>> waits;
  if (!one_shot) for (Engine* e : order) waits.emplace_back(e->long_call_mu);
  std::vector<eg_ctx*> ctxs;
  for (Engine* e : engines) if (std::find(ctxs.begin(), ctxs.end(), e->ctx) == ctxs.end()) ctxs.push_back(e->ctx);
  std::sort(ctxs.begin(), ctxs.end(), std::less<eg_ctx*>());
  LockAll lk(ctxs);
  for (Engine* e : engines)
    if (e->stream_open) return fail(EG_ERR_BAD_ARG, one_shot ? "a JSON stream is open on this params object (eg_verify_json_end or _abort it first)"
                                                             : "a JSON stream is already open on this params object");
  TRY(stream_begin(engines, threads, std::move(pack_piece), std::move(reshape), size_hint, out));
  (*out)->one_shot = one_shot;
  (*out)->max_objects = max_objects;              // one-shot: the worker breaks off as soon as the text holds more (nothing further is parsed or verified)
  return EG_OK;
}
// The one-shot entry = the streaming entry fed with the whole text (in place, 64 MB at a time) - one pipeline for both (round 5; rounds 3-4
// had a second one here, a producer thread and a consumer loop over the same ring).
static int verify_json_common(const std::vector<Engine*>& engines, const char* json, size_t json_len, int threads, size_t max_objects, uint32_t* status,
                              size_t* n_objects, uint8_t* tally_out, const PackPieceFn& pack_piece, const ReshapeFn& reshape) {
  if ((json_len && !json) || (max_objects && !status)) return fail(EG_ERR_BAD_ARG, "bad argument");
  if (n_objects) *n_objects = 0;
  eg_json_stream* S = nullptr;
  // concurrent long calls on a params object are serialised, as every entry point is: the call holds every engine's long_call_mu (address order)
  std::vector<Engine*> order(engines);
  std::sort(order.begin(), order.end(), std::less<Engine*>());
  std::vector<std::unique_lock<std::mutex>> one_at_a_time;
  for (Engine* e : order) one_at_a_time.emplace_back(e->long_call_mu);
  // the contexts' locks only while the stream is opened: its worker thread takes them piece by piece, and so does end
  TRY(stream_open_on(engines, threads, pack_piece, reshape, json_len, true, max_objects, &S));
  const size_t piece = (size_t)64 << 20;
  for (size_t at = 0; at < json_len; at += piece) {
    if (eg_verify_json_feed(S, json + at, std::min(piece, json_len - at), nullptr)) break;       // end reports it and cleans up
  }
  size_t taken = 0, total = 0;
  const int rc = eg_verify_json_end(S, status, max_objects, &taken, &total, tally_out);
  // end leaves the stream OPEN in exactly one case - more verdicts are left than `status` has room for - and says so through its
  // out-values: *n_taken = the number left (> cap).  Every other failure has destroyed the stream and reports *n_taken = 0.  (The worker
  // normally fails the stream as soon as it has cut more than max_objects values, long before this point: stream_emit.)
  if (rc == EG_ERR_BAD_ARG && taken > max_objects) {
    eg_verify_json_abort(S);
    return fail(EG_ERR_BAD_ARG, "more objects in the text than max_objects");
  }
  if (rc) return rc;
  if (n_objects) *n_objects = total;
  return EG_OK;
}
// how a choice / QV election packs its ballots and resolves the ones of another shape (the object path runs on the FIRST engine)
static void choice_json_fns(const eg_choice_params* p, PackPieceFn* pack, ReshapeFn* reshape) {
  const int n_options = p->n_options, single = p->single;
  const size_t stride = p->eng->plan.stride;
  Engine* e = p->eng;
  *pack = [=](const char* text, const std::vector<std::pair<size_t, size_t>>& sub, int th, uint8_t* dst, uint32_t* st, egwire::WorkerPool* pool) {
    egwire::pack_parallel(text, sub, stride, th, dst, st, [&](egwire::Cursor& c, uint8_t* d) { return egwire::pack_choice(c, n_options, single != 0, d); }, pool);
  };
  *reshape = [=](const char* text, const std::vector<std::pair<size_t, size_t>>& odd, std::vector<uint32_t>& res) {
    return egwire::resolve_choice_objects(text, odd, n_options, single != 0, stride, make_check_items(e->ctx), make_verify_packed(e), res);
  };
}
static void qv_json_fns(const eg_qv_params* p, PackPieceFn* pack, ReshapeFn* reshape) {
  const int n_options = p->n_options;
  const eghost::QvShape sh = p->shape;
  const egwire::RangeShape vote{sh.vote_range.rings.size(), (size_t)sh.vote_range.rings_size()};
  const egwire::RangeShape credit{sh.credit_range.rings.size(), (size_t)sh.credit_range.rings_size()};
  Engine* e = p->eng;
  *pack = [=](const char* text, const std::vector<std::pair<size_t, size_t>>& sub, int th, uint8_t* dst, uint32_t* st, egwire::WorkerPool* pool) {
    egwire::pack_parallel(text, sub, sh.ballot_size, th, dst, st, [&](egwire::Cursor& c, uint8_t* d) { return egwire::pack_qv(c, n_options, vote, credit, sh.ballot_size, d); }, pool);
  };
  *reshape = [=](const char* text, const std::vector<std::pair<size_t, size_t>>& odd, std::vector<uint32_t>& res) {
    return egwire::resolve_qv_objects(text, odd, n_options, vote, credit, sh.ballot_size, make_check_items(e->ctx), make_verify_packed(e), res);
  };
}
extern "C++" {
template <class Params>
static int engines_of(Params* const* per_device, int n_dev, std::vector<Engine*>* out) {
  TRY(multi_check(per_device, n_dev));
  for (int d = 0; d < n_dev; ++d) out->push_back(per_device[d]->eng);
  return EG_OK;
}
}
int eg_verify_choice_json(eg_choice_params* p, const char* json, size_t json_len, int threads, size_t max_objects, uint32_t* status,
                          size_t* n_objects, uint8_t* tally_out) {
  if (!p) return fail(EG_ERR_BAD_ARG, "bad argument");
  PackPieceFn pack; ReshapeFn reshape;
  choice_json_fns(p, &pack, &reshape);
  return verify_json_common({p->eng}, json, json_len, threads, max_objects, status, n_objects, tally_out, pack, reshape);
}
int eg_verify_qv_json(eg_qv_params* p, const char* json, size_t json_len, int threads, size_t max_objects, uint32_t* status,
                      size_t* n_objects, uint8_t* tally_out) {
  if (!p) return fail(EG_ERR_BAD_ARG, "bad argument");
  PackPieceFn pack; ReshapeFn reshape;
  qv_json_fns(p, &pack, &reshape);
  return verify_json_common({p->eng}, json, json_len, threads, max_objects, status, n_objects, tally_out, pack, reshape);
}
int eg_verify_choice_json_multi(eg_choice_params* const* per_device, int n_dev, const char* json, size_t json_len, int threads, size_t max_objects,
                                uint32_t* status, size_t* n_objects, uint8_t* tally_out) {
  std::vector<Engine*> engines;
  TRY(engines_of(per_device, n_dev, &engines));
  PackPieceFn pack; ReshapeFn reshape;
  choice_json_fns(per_device[0], &pack, &reshape);
  return verify_json_common(engines, json, json_len, threads, max_objects, status, n_objects, tally_out, pack, reshape);
}
int eg_verify_qv_json_multi(eg_qv_params* const* per_device, int n_dev, const char* json, size_t json_len, int threads, size_t max_objects,
                            uint32_t* status, size_t* n_objects, uint8_t* tally_out) {
  std::vector<Engine*> engines;
  TRY(engines_of(per_device, n_dev, &engines));
  PackPieceFn pack; ReshapeFn reshape;
  qv_json_fns(per_device[0], &pack, &reshape);
  return verify_json_common(engines, json, json_len, threads, max_objects, status, n_objects, tally_out, pack, reshape);
}
int eg_verify_choice_json_begin(eg_choice_params* p, int threads, eg_json_stream** out) {
  if (!p) return fail(EG_ERR_BAD_ARG, "bad argument");
  PackPieceFn pack; ReshapeFn reshape;
  choice_json_fns(p, &pack, &reshape);
  return stream_open_on({p->eng}, threads, pack, reshape, 0, false, (size_t)-1, out);
}
int eg_verify_qv_json_begin(eg_qv_params* p, int threads, eg_json_stream** out) {
  if (!p) return fail(EG_ERR_BAD_ARG, "bad argument");
  PackPieceFn pack; ReshapeFn reshape;
  qv_json_fns(p, &pack, &reshape);
  return stream_open_on({p->eng}, threads, pack, reshape, 0, false, (size_t)-1, out);
}
int eg_verify_choice_json_begin_multi(eg_choice_params* const* per_device, int n_dev, int threads, eg_json_stream** out) {
  std::vector<Engine*> engines;
  TRY(engines_of(per_device, n_dev, &engines));
  PackPieceFn pack; ReshapeFn reshape;
  choice_json_fns(per_device[0], &pack, &reshape);
  return stream_open_on(engines, threads, pack, reshape, 0, false, (size_t)-1, out);
}
int eg_verify_qv_json_begin_multi(eg_qv_params* const* per_device, int n_dev, int threads, eg_json_stream** out) {
  std::vector<Engine*> engines;
  TRY(engines_of(per_device, n_dev, &engines));
  PackPieceFn pack; ReshapeFn reshape;
  qv_json_fns(per_device[0], &pack, &reshape);
  return stream_open_on(engines, threads, pack, reshape, 0, false, (size_t)-1, out);
}
size_t eg_qv_ballot_size_for(int n_options, uint64_t credits) {
  if (n_options < 1 || n_options > 256 || credits < 1 || credits > 100000) return 0;
  return eghost::qv_shape(n_options, credits).ballot_size;
}

// ---- synthetic ballots ---------------------------------------------------------------------------------------------------------
// what EncryptedChoice::single / ::new would refuse or mis-prove (the host forms of the generator and of the opener)
static int check_selection(const eg_choice_params* p, size_t n, const uint32_t* selection) {
  const size_t sw = ((size_t)p->n_options + 31) / 32;
  for (size_t i = 0; i < n; ++i) {
    int chosen = 0;
    for (size_t w = 0; w < sw; ++w) {
      const uint32_t word = selection[i * sw + w];
      const int valid_bits = (int)std::min<size_t>(32, (size_t)p->n_options - 32 * w);
      if (valid_bits < 32 && (word >> valid_bits)) return fail(EG_ERR_BAD_ARG, "selection has bits beyond the options");
      chosen += __builtin_popcount(word);
    }
    if (p->single && chosen != 1) return fail(EG_ERR_BAD_ARG, "a single-choice ballot selects exactly one option");
  }
  return EG_OK;
}
// the assertions of QuadraticVotingBallot::new (quadratic_voting.rs:240-253)
static int check_votes(const eg_qv_params* p, size_t n, const uint32_t* votes) {
  const uint64_t max_vote = eghost::isqrt(p->credits);
  for (size_t i = 0; i < n; ++i) {
    uint64_t credit = 0;
    for (int k = 0; k < p->n_options; ++k) {
      const uint64_t v = votes[i * (size_t)p->n_options + k];
      if (v > max_vote) return fail(EG_ERR_BAD_ARG, "a vote exceeds isqrt(credits)");
      credit += v * v;
    }
    if (credit > p->credits) return fail(EG_ERR_BAD_ARG, "votes exceed the credit amount");
  }
  return EG_OK;
}
static int choice_encrypt_device(eg_choice_params* p, uint64_t base_seed, size_t first, size_t n, int n_selected,
                                 const void* d_selection, uint64_t rng_skip, void* d_out, hipStream_t s) {
  Engine* e = p->eng;
  HIPCHK(hipSetDevice(e->ctx->device));
  if (!d_selection && !p->single && (n_selected < 0 || n_selected > p->n_options)) return fail(EG_ERR_BAD_ARG, "n_selected out of range");
  if (n == 0) return EG_OK;
  int blocks = 0;
  TRY(gen_workspace(e, n, eg_gen_choice_ws_words(p->n_options), &blocks));
  eg_launch_choice_encrypt(blocks, s, base_seed + first, n, p->n_options, p->single, n_selected,
                           reinterpret_cast<const u32*>(d_selection), rng_skip, e->ctx->tabG,
                           e->d_tabK, e->d_prefixes, e->plan.gen_pre_main, e->plan.gen_pre_ring, e->plan.gen_pre_logeq,
                           reinterpret_cast<u32*>(d_out), (u32)(e->plan.stride / 4), e->gen_ws);
  HIPCHK(hipGetLastError());
  return EG_OK;
}
int eg_choice_encrypt_batch_device(eg_choice_params* p, uint64_t base_seed, size_t first, size_t n, int n_selected, void* d_out,
                                   void* stream) { EG_LOCK_P(p);
  if (!p || (n && !d_out)) return fail(EG_ERR_BAD_ARG, "bad argument");
  return choice_encrypt_device(p, base_seed, first, n, n_selected, nullptr, 0, d_out, (hipStream_t)stream);
}
int eg_choice_encrypt_batch(eg_choice_params* p, uint64_t base_seed, size_t first, size_t n, int n_selected, uint8_t* out) { EG_LOCK_P(p);
  if (!p || (n && !out)) return fail(EG_ERR_BAD_ARG, "bad argument");
  Engine* e = p->eng;
  HIPCHK(hipSetDevice(e->ctx->device));
  DevBuf d;
  TRY(d.alloc(n * e->plan.stride));
  TRY(choice_encrypt_device(p, base_seed, first, n, n_selected, nullptr, 0, d.p, e->ctx->stream));
  TRY(d.get(out, n * e->plan.stride, e->ctx->stream));
  HIPCHK(hipStreamSynchronize(e->ctx->stream));
  return EG_OK;
}
int eg_choice_encrypt_selected_batch_device(eg_choice_params* p, uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip,
                                            const void* d_selection, void* d_out, void* stream) { EG_LOCK_P(p);
  if (!p || (n && (!d_out || !d_selection))) return fail(EG_ERR_BAD_ARG, "bad argument");
  return choice_encrypt_device(p, base_seed, first, n, 0, d_selection, rng_skip, d_out, (hipStream_t)stream);
}
int eg_choice_encrypt_selected_batch(eg_choice_params* p, uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip,
                                     const uint32_t* selection, uint8_t* out) { EG_LOCK_P(p);
  if (!p || (n && (!out || !selection))) return fail(EG_ERR_BAD_ARG, "bad argument");
  Engine* e = p->eng;
  HIPCHK(hipSetDevice(e->ctx->device));
  const size_t sw = ((size_t)p->n_options + 31) / 32;
  TRY(check_selection(p, n, selection));
  DevBuf d, sel;
  TRY(d.alloc(n * e->plan.stride)); TRY(sel.alloc(n * sw * 4));
  TRY(sel.put(selection, n * sw * 4, e->ctx->stream));
  TRY(choice_encrypt_device(p, base_seed, first, n, 0, sel.p, rng_skip, d.p, e->ctx->stream));
  TRY(d.get(out, n * e->plan.stride, e->ctx->stream));
  HIPCHK(hipStreamSynchronize(e->ctx->stream));
  return EG_OK;
}
static int qv_encrypt_device(eg_qv_params* p, uint64_t base_seed, size_t first, size_t n, const void* d_votes, uint64_t rng_skip,
                             void* d_out, hipStream_t s) {
  Engine* e = p->eng;
  HIPCHK(hipSetDevice(e->ctx->device));
  const eghost::QvShape& sh = p->shape;
  if (n == 0) return EG_OK;
  const size_t vr = sh.vote_range.rings.size(), cr = sh.credit_range.rings.size();
  if (!e->d_gen_desc) {     // ring shapes (size, step) of the vote range, then of the credit range
    std::vector<u32> desc;
    for (auto* d : {&sh.vote_range, &sh.credit_range})
      for (auto& r : d->rings) { desc.push_back((u32)r.size); desc.push_back((u32)r.step); }
    HIPCHK(hipMalloc((void**)&e->d_gen_desc, desc.size() * sizeof(u32)));
    HIPCHK(hipMemcpy(e->d_gen_desc, desc.data(), desc.size() * sizeof(u32), hipMemcpyHostToDevice));
  }
  int blocks = 0;
  const unsigned words = eg_gen_qv_ws_words(p->n_options, (unsigned)std::max(vr, cr),
                                            (unsigned)std::max(sh.vote_range.rings_size(), sh.credit_range.rings_size()));
  TRY(gen_workspace(e, n, words, &blocks));
  eg_launch_qv_encrypt(blocks, s, base_seed + first, n, p->n_options, p->credits, reinterpret_cast<const u32*>(d_votes), rng_skip,
                       (int)vr, e->plan.gen_vote_main, e->plan.gen_vote_ring, e->d_gen_desc, (int)cr, e->plan.gen_credit_main,
                       e->plan.gen_credit_ring, e->d_gen_desc + 2 * vr, e->plan.gen_pre_sumsq, e->ctx->tabG, e->d_tabK,
                       e->d_prefixes, reinterpret_cast<u32*>(d_out), (u32)(sh.ballot_size / 4), (u32)(sh.vote_size / 4),
                       (u32)(sh.credit_size / 4), e->gen_ws);
  HIPCHK(hipGetLastError());
  return EG_OK;
}
int eg_qv_encrypt_batch_device(eg_qv_params* p, uint64_t base_seed, size_t first, size_t n, void* d_out, void* stream) { EG_LOCK_P(p);
  if (!p || (n && !d_out)) return fail(EG_ERR_BAD_ARG, "bad argument");
  return qv_encrypt_device(p, base_seed, first, n, nullptr, 0, d_out, (hipStream_t)stream);
}
int eg_qv_encrypt_votes_batch_device(eg_qv_params* p, uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip,
                                     const void* d_votes, void* d_out, void* stream) { EG_LOCK_P(p);
  if (!p || (n && (!d_out || !d_votes))) return fail(EG_ERR_BAD_ARG, "bad argument");
  return qv_encrypt_device(p, base_seed, first, n, d_votes, rng_skip, d_out, (hipStream_t)stream);
}
int eg_qv_encrypt_votes_batch(eg_qv_params* p, uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip, const uint32_t* votes,
                              uint8_t* out) { EG_LOCK_P(p);
  if (!p || (n && (!out || !votes))) return fail(EG_ERR_BAD_ARG, "bad argument");
  Engine* e = p->eng;
  HIPCHK(hipSetDevice(e->ctx->device));
  TRY(check_votes(p, n, votes));
  DevBuf d, vv;
  TRY(d.alloc(n * e->plan.stride)); TRY(vv.alloc(n * (size_t)p->n_options * 4));
  TRY(vv.put(votes, n * (size_t)p->n_options * 4, e->ctx->stream));
  TRY(qv_encrypt_device(p, base_seed, first, n, vv.p, rng_skip, d.p, e->ctx->stream));
  TRY(d.get(out, n * e->plan.stride, e->ctx->stream));
  HIPCHK(hipStreamSynchronize(e->ctx->stream));
  return EG_OK;
}

// ---- ballot audits (Benaloh challenge): opened ballots against their ciphertexts (open_kernels.cuh), and the opener of synthetic ballots ----
// Stateless like weeding: the plan's immutable data (stride, tally items) and the narrow comb tables of G and K only - no lock, no
// workspace, no running tally, any stream.
static uint32_t open_slots(const Engine* e) { return (uint32_t)(e->plan.tally_slots.size() / 2); }
static size_t open_check_scratch_bytes(const Engine* e, size_t n) {
  if (!e || !e->weed_keys_ok || n >= ego::N_LIMIT || ego::refuse_items(n, open_slots(e))) return 0;
  return ego::layout(n, open_slots(e)).total;
}
// the argument rules, in the order the header gives them; nothing of the params object is looked at before they hold
static int open_check_args(const Engine* e, size_t n, const ego::Have& h) {
  const char* why = ego::refuse(n, h);
  if (why) return fail(EG_ERR_BAD_ARG, std::string("open check: ") + why);
  if (!e) return fail(EG_ERR_BAD_ARG, "open check: null params");
  if (!e->weed_keys_ok) return fail(EG_ERR_BAD_ARG, "open check: internal: the tally ciphertexts of this plan are not contiguous wire items");
  if ((why = ego::refuse_items(n, open_slots(e)))) return fail(EG_ERR_BAD_ARG, std::string("open check: ") + why);
  return EG_OK;
}
static int open_check_launch(Engine* e, size_t n, const void* d_ballots, const void* d_status_in, const void* d_values, const void* d_rand,
                             void* d_status_out, void* d_found, void* d_scratch, hipStream_t s) {
  if (const char* why = ego::refuse(n, ego::Have{d_ballots != nullptr, d_values != nullptr, d_rand != nullptr, d_status_out != nullptr, d_found != nullptr}))
    return fail(EG_ERR_BAD_ARG, std::string("open check: ") + why);
  if (const char* why = ego::refuse_alignment((uintptr_t)d_ballots | (uintptr_t)d_scratch, (uintptr_t)d_values,
                                              (uintptr_t)d_rand | (uintptr_t)d_status_in | (uintptr_t)d_status_out | (uintptr_t)d_found))
    return fail(EG_ERR_BAD_ARG, std::string("open check: ") + why);
  TRY_(open_check_args(e, n, ego::Have{true, true, true, true, true}));
  const u32 n_slots = open_slots(e);
  const ego::Layout L = ego::layout(n, n_slots);
  if (L.total && !d_scratch) return fail(EG_ERR_BAD_ARG, "open check: null scratch (eg_*_open_check_scratch_bytes says how much)");
  if (!d_found) return EG_OK;                                            // n == 0 and nowhere to write anything to
  HIPCHK(hipSetDevice(e->ctx->device));
  u32* found = static_cast<u32*>(d_found);
  HIPCHK(hipMemsetAsync(found, 0, 2 * sizeof(u32), s));
  if (n) {
    u32* words = reinterpret_cast<u32*>(static_cast<char*>(d_scratch) + L.words);
    const u32* status = static_cast<const u32*>(d_status_in);
    const OpenMemDev mem{static_cast<const uint8_t*>(d_ballots), (const u32*)e->d_tally_items, (u64)e->plan.stride,
                         static_cast<const unsigned long long*>(d_values), static_cast<const u32*>(d_rand), words};
    const size_t items = n * (size_t)n_slots;
    hipLaunchKernelGGL(k_open_check, dim3((unsigned)((items + NT - 1) / NT)), dim3(NT), 0, s, mem, status, (u64)n, n_slots,
                       (const uint4*)e->ctx->tabG, (const uint4*)e->d_tabK, words);
    hipLaunchKernelGGL(k_open_resolve, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, s, mem, status, (u64)n, n_slots,
                       static_cast<u32*>(d_status_out), found);
  }
  HIPCHK(hipGetLastError());
  return EG_OK;
}
static int open_check_host(Engine* e, size_t n, const uint8_t* ballots, const uint32_t* status_in, const uint64_t* values, const uint8_t* rand,
                           uint32_t* status_out, uint32_t* found) {
  TRY_(open_check_args(e, n, ego::Have{ballots != nullptr, values != nullptr, rand != nullptr, status_out != nullptr, found != nullptr}));
  if (found) found[0] = found[1] = 0;
  if (n == 0) return EG_OK;
  HIPCHK(hipSetDevice(e->ctx->device));
  const size_t items = n * (size_t)open_slots(e);
  HostStage st("open check"); TRY_(st.open());
  void *db, *dsi = nullptr, *dv, *dr, *dso, *dfound, *scratch;
  TRY_(st.put(&db, ballots, n * e->plan.stride));
  if (status_in) TRY_(st.put(&dsi, status_in, n * 4));
  TRY_(st.put(&dv, values, items * 8));
  TRY_(st.put(&dr, rand, items * ego::RAND_BYTES));
  TRY_(st.put(&dso, nullptr, n * 4));
  TRY_(st.put(&dfound, nullptr, 2 * 4));
  TRY_(st.put(&scratch, nullptr, open_check_scratch_bytes(e, n)));
  TRY_(open_check_launch(e, n, db, dsi, dv, dr, dso, dfound, scratch, st.s));
  TRY_(st.get(status_out, dso, n * 4));
  TRY_(st.get(found, dfound, 2 * 4));
  TRY_(st.sync());
  return EG_OK;
}
size_t eg_choice_open_check_scratch_bytes(const eg_choice_params* p, size_t n) { return open_check_scratch_bytes(p ? p->eng : nullptr, n); }
size_t eg_qv_open_check_scratch_bytes(const eg_qv_params* p, size_t n) { return open_check_scratch_bytes(p ? p->eng : nullptr, n); }
int eg_choice_open_check_device(eg_choice_params* p, size_t n, const void* d_ballots, const void* d_status_in, const void* d_values,
                                const void* d_rand, void* d_status_out, void* d_found, void* d_scratch, void* stream) {
  return open_check_launch(p ? p->eng : nullptr, n, d_ballots, d_status_in, d_values, d_rand, d_status_out, d_found, d_scratch, (hipStream_t)stream);
}
int eg_qv_open_check_device(eg_qv_params* p, size_t n, const void* d_ballots, const void* d_status_in, const void* d_values, const void* d_rand,
                            void* d_status_out, void* d_found, void* d_scratch, void* stream) {
  return open_check_launch(p ? p->eng : nullptr, n, d_ballots, d_status_in, d_values, d_rand, d_status_out, d_found, d_scratch, (hipStream_t)stream);
}
int eg_choice_open_check(eg_choice_params* p, size_t n, const uint8_t* ballots, const uint32_t* status_in, const uint64_t* values,
                         const uint8_t* rand, uint32_t* status_out, uint32_t* found) {
  return open_check_host(p ? p->eng : nullptr, n, ballots, status_in, values, rand, status_out, found);
}
int eg_qv_open_check(eg_qv_params* p, size_t n, const uint8_t* ballots, const uint32_t* status_in, const uint64_t* values, const uint8_t* rand,
                     uint32_t* status_out, uint32_t* found) {
  return open_check_host(p ? p->eng : nullptr, n, ballots, status_in, values, rand, status_out, found);
}

// The opener (open_gen_kernels.cuh): no lock and no workspace either - it reads the shape of the election and nothing else.
static int open_batch_args(const Engine* e, size_t n, const void* values_out, const void* rand_out) {
  if (n >= ego::N_LIMIT) return fail(EG_ERR_BAD_ARG, "open batch: n is 2^31 or more");
  if (n && (!values_out || !rand_out)) return fail(EG_ERR_BAD_ARG, "open batch: null values_out or rand_out");
  if (const char* why = ego::refuse_alignment(0, (uintptr_t)values_out, (uintptr_t)rand_out)) return fail(EG_ERR_BAD_ARG, std::string("open batch: ") + why);
  if (!e) return fail(EG_ERR_BAD_ARG, "open batch: null params");
  if (const char* why = ego::refuse_items(n, open_slots(e))) return fail(EG_ERR_BAD_ARG, std::string("open batch: ") + why);
  return EG_OK;
}
static int choice_open_device(eg_choice_params* p, uint64_t base_seed, size_t first, size_t n, int n_selected, uint64_t rng_skip,
                              const void* d_selection, void* d_values_out, void* d_rand_out, hipStream_t s) {
  TRY_(open_batch_args(p ? p->eng : nullptr, n, d_values_out, d_rand_out));
  if ((uintptr_t)d_selection & 3u) return fail(EG_ERR_BAD_ARG, "open batch: selection must be 4-byte aligned");
  if (!d_selection && !p->single && (n_selected < 0 || n_selected > p->n_options)) return fail(EG_ERR_BAD_ARG, "open batch: n_selected out of range");
  if (n == 0) return EG_OK;
  Engine* e = p->eng;
  HIPCHK(hipSetDevice(e->ctx->device));
  eg_launch_choice_open(grid_for(n, e->ctx->cus * 4), s, base_seed + first, n, p->n_options, p->single, n_selected,
                        static_cast<const u32*>(d_selection), rng_skip, static_cast<unsigned long long*>(d_values_out), static_cast<u32*>(d_rand_out));
  HIPCHK(hipGetLastError());
  return EG_OK;
}
static int qv_open_device(eg_qv_params* p, uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip, const void* d_votes, void* d_values_out,
                          void* d_rand_out, hipStream_t s) {
  TRY_(open_batch_args(p ? p->eng : nullptr, n, d_values_out, d_rand_out));
  if ((uintptr_t)d_votes & 3u) return fail(EG_ERR_BAD_ARG, "open batch: votes must be 4-byte aligned");
  if (n == 0) return EG_OK;
  Engine* e = p->eng;
  HIPCHK(hipSetDevice(e->ctx->device));
  const eghost::RangeDecomposition& vr = p->shape.vote_range;
  eg_launch_qv_open(grid_for(n, e->ctx->cus * 4), s, base_seed + first, n, p->n_options, p->credits, static_cast<const u32*>(d_votes), rng_skip,
                    ego::range_draws((u32)vr.rings.size(), vr.rings_size()), static_cast<unsigned long long*>(d_values_out),
                    static_cast<u32*>(d_rand_out));
  HIPCHK(hipGetLastError());
  return EG_OK;
}
// host arrays: `choices` = the selection or the votes (null: drawn from the second stream), `per_ballot` words of it a ballot
static int open_batch_host(const Engine* e, size_t n, const uint32_t* choices, size_t per_ballot, uint64_t* values_out, uint8_t* rand_out,
                           const std::function<int(void*, void*, void*, hipStream_t)>& launch) {
  TRY_(open_batch_args(e, n, values_out, rand_out));
  if (n == 0) return EG_OK;
  HIPCHK(hipSetDevice(e->ctx->device));
  const size_t items = n * (size_t)open_slots(e);
  HostStage st("open batch"); TRY_(st.open());
  void *dc = nullptr, *dv, *dr;
  if (choices) TRY_(st.put(&dc, choices, n * per_ballot * 4));
  TRY_(st.put(&dv, nullptr, items * 8));
  TRY_(st.put(&dr, nullptr, items * ego::RAND_BYTES));
  TRY_(launch(dc, dv, dr, st.s));
  TRY_(st.get(values_out, dv, items * 8));
  TRY_(st.get(rand_out, dr, items * ego::RAND_BYTES));
  TRY_(st.sync());
  return EG_OK;
}
int eg_choice_open_batch_device(eg_choice_params* p, uint64_t base_seed, size_t first, size_t n, int n_selected, uint64_t rng_skip,
                                const void* d_selection, void* d_values_out, void* d_rand_out, void* stream) {
  return choice_open_device(p, base_seed, first, n, n_selected, rng_skip, d_selection, d_values_out, d_rand_out, (hipStream_t)stream);
}
int eg_choice_open_batch(eg_choice_params* p, uint64_t base_seed, size_t first, size_t n, int n_selected, uint64_t rng_skip,
                         const uint32_t* selection, uint64_t* values_out, uint8_t* rand_out) {
  TRY_(open_batch_args(p ? p->eng : nullptr, n, values_out, rand_out));
  if (selection) TRY_(check_selection(p, n, selection));
  return open_batch_host(p->eng, n, selection, ((size_t)p->n_options + 31) / 32, values_out, rand_out,
                         [&](void* dc, void* dv, void* dr, hipStream_t s) { return choice_open_device(p, base_seed, first, n, n_selected, rng_skip, dc, dv, dr, s); });
}
int eg_qv_open_batch_device(eg_qv_params* p, uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip, const void* d_votes,
                            void* d_values_out, void* d_rand_out, void* stream) {
  return qv_open_device(p, base_seed, first, n, rng_skip, d_votes, d_values_out, d_rand_out, (hipStream_t)stream);
}
int eg_qv_open_batch(eg_qv_params* p, uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip, const uint32_t* votes,
                     uint64_t* values_out, uint8_t* rand_out) {
  TRY_(open_batch_args(p ? p->eng : nullptr, n, values_out, rand_out));
  if (votes) TRY_(check_votes(p, n, votes));
  return open_batch_host(p->eng, n, votes, (size_t)p->n_options, values_out, rand_out,
                         [&](void* dc, void* dv, void* dr, hipStream_t s) { return qv_open_device(p, base_seed, first, n, rng_skip, dc, dv, dr, s); });
}

// CommitmentEquivalenceProof::new per item (prover_kernels.cuh: k_commit_equiv_prove), over the narrow comb tables of G, K and H
static int commit_equiv_prove_device(eg_proof_params* p, uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip, const void* d_values,
                                     void* d_items, void* d_blindings, hipStream_t s) {
  Engine* e = p->eng;
  if (p->kind != EG_PROOF_COMMIT_EQUIV || !e->d_tabH) return fail(EG_ERR_BAD_ARG, "not a commitment-equivalence params object");
  HIPCHK(hipSetDevice(e->ctx->device));
  if (n == 0) return EG_OK;
  eg_launch_commit_equiv_prove(grid_for(n, e->ctx->cus * 4), s, base_seed + first, n, rng_skip, reinterpret_cast<const u64*>(d_values),
                               e->ctx->tabG, e->d_tabK, e->d_tabH, e->d_prefixes, e->plan.gen_pre_cequiv, reinterpret_cast<u32*>(d_items),
                               reinterpret_cast<u32*>(d_blindings));
  HIPCHK(hipGetLastError());
  return EG_OK;
}
int eg_commit_equiv_prove_batch_device(eg_proof_params* p, uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip, const void* d_values,
                                       void* d_items, void* d_blindings, void* stream) { EG_LOCK_P(p);
  if (!p || (n && (!d_values || !d_items))) return fail(EG_ERR_BAD_ARG, "bad argument");
  return commit_equiv_prove_device(p, base_seed, first, n, rng_skip, d_values, d_items, d_blindings, (hipStream_t)stream);
}
int eg_commit_equiv_prove_batch(eg_proof_params* p, uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip, const uint64_t* values,
                                uint8_t* items, uint8_t* blindings) { EG_LOCK_P(p);
  if (!p || (n && (!values || !items))) return fail(EG_ERR_BAD_ARG, "bad argument");
  Engine* e = p->eng;
  HIPCHK(hipSetDevice(e->ctx->device));
  DevBuf v, d, b;
  TRY(v.alloc(n * 8)); TRY(d.alloc(n * eghost::COMMIT_EQUIV_ITEM)); TRY(b.alloc(n * 32));
  TRY(v.put(values, n * 8, e->ctx->stream));
  TRY(commit_equiv_prove_device(p, base_seed, first, n, rng_skip, v.p, d.p, blindings ? b.p : nullptr, e->ctx->stream));
  TRY(d.get(items, n * eghost::COMMIT_EQUIV_ITEM, e->ctx->stream));
  if (blindings) TRY(b.get(blindings, n * 32, e->ctx->stream));
  HIPCHK(hipStreamSynchronize(e->ctx->stream));
  return EG_OK;
}

// ---- provers of the single-item proofs (prover_kernels.cuh: k_zero_prove, k_range_prove, k_sumsq_prove, k_share_prove) ----------------
static_assert(EG_PROOF_ZERO == eghost::PROVE_ZERO && EG_PROOF_BOOL == eghost::PROVE_BOOL && EG_PROOF_RANGE == eghost::PROVE_RANGE &&
              EG_PROOF_SHARE == eghost::PROVE_SHARE && EG_PROOF_SUMSQ == eghost::PROVE_SUMSQ, "host_plan.hpp names the kinds of eg_hip.h");
size_t eg_proof_prove_input_size(const eg_proof_params* p) {
  const int per = p ? eghost::prove_inputs_per_item(p->kind, p->n_values) : -1;
  return per < 0 ? 0 : (size_t)per * 8;
}
static int proof_prove_device(eg_proof_params* p, uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip, const void* d_inputs,
                              void* d_items, hipStream_t s) {
  Engine* e = p->eng;
  HIPCHK(hipSetDevice(e->ctx->device));
  if (n == 0) return EG_OK;
  const u64* vals = reinterpret_cast<const u64*>(d_inputs);
  u32* out = reinterpret_cast<u32*>(d_items);
  int blocks = 0;
  if (p->kind == EG_PROOF_ZERO) {
    eg_launch_zero_prove(grid_for(n, e->ctx->cus * 4), s, base_seed + first, n, rng_skip, e->ctx->tabG, e->d_tabK, e->d_prefixes,
                         e->plan.gen_pre_logeq, out);
  } else if (p->kind == EG_PROOF_SUMSQ) {
    TRY(gen_workspace(e, n, egplan::gen_sumsq_ws_words((u32)p->n_values), &blocks));
    eg_launch_sumsq_prove(blocks, s, base_seed + first, n, rng_skip, p->n_values, vals, e->plan.gen_pre_sumsq, e->ctx->tabG, e->d_tabK,
                          e->d_prefixes, out, (u32)(p->item_size / 4), e->gen_ws);
  } else {     // bool and range: RangeProof::new over the object's decomposition
    const auto& rings = p->range.rings;
    if (!e->d_gen_desc) {
      std::vector<u32> desc;
      for (auto& r : rings) { desc.push_back((u32)r.size); desc.push_back((u32)r.step); }
      HIPCHK(hipMalloc((void**)&e->d_gen_desc, desc.size() * sizeof(u32)));
      HIPCHK(hipMemcpy(e->d_gen_desc, desc.data(), desc.size() * sizeof(u32), hipMemcpyHostToDevice));
    }
    TRY(gen_workspace(e, n, egplan::gen_range_ws_words((u32)rings.size(), (u32)p->range.rings_size()), &blocks));
    eg_launch_range_prove(blocks, s, base_seed + first, n, rng_skip, vals, (int)rings.size(), e->plan.gen_pre_main, e->plan.gen_pre_ring,
                          e->d_gen_desc, e->ctx->tabG, e->d_tabK, e->d_prefixes, out, (u32)(p->item_size / 4), e->gen_ws);
  }
  HIPCHK(hipGetLastError());
  return EG_OK;
}
static int proof_prove_kind_ok(const eg_proof_params* p) {
  if (eghost::prove_inputs_per_item(p->kind, p->n_values) < 0)
    return fail(EG_ERR_BAD_ARG, p->kind == EG_PROOF_SHARE ? "a decryption share needs the secret share: eg_share_prove_batch"
                                                          : "commitment-equivalence proofs have their own entry: eg_commit_equiv_prove_batch");
  return EG_OK;
}
int eg_proof_prove_batch_device(eg_proof_params* p, uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip, const void* d_inputs,
                                void* d_items, void* stream) { EG_LOCK_P(p);
  if (!p) return fail(EG_ERR_BAD_ARG, "bad argument");
  TRY(proof_prove_kind_ok(p));
  if (n && (!d_items || (!d_inputs && p->kind != EG_PROOF_ZERO))) return fail(EG_ERR_BAD_ARG, "bad argument");
  return proof_prove_device(p, base_seed, first, n, rng_skip, d_inputs, d_items, (hipStream_t)stream);
}
int eg_proof_prove_batch(eg_proof_params* p, uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip, const uint64_t* inputs,
                         uint8_t* items) { EG_LOCK_P(p);
  if (!p) return fail(EG_ERR_BAD_ARG, "bad argument");
  TRY(proof_prove_kind_ok(p));
  if (n && (!items || (!inputs && p->kind != EG_PROOF_ZERO))) return fail(EG_ERR_BAD_ARG, "bad argument");
  if (const char* why = eghost::check_prove_inputs(p->kind, p->upper_bound, p->n_values, inputs, n)) return fail(EG_ERR_BAD_ARG, why);
  Engine* e = p->eng;
  HIPCHK(hipSetDevice(e->ctx->device));
  const size_t in_bytes = n * eg_proof_prove_input_size(p);
  DevBuf v, d;
  TRY(v.alloc(in_bytes)); TRY(d.alloc(n * p->item_size));
  TRY(v.put(inputs, in_bytes, e->ctx->stream));
  TRY(proof_prove_device(p, base_seed, first, n, rng_skip, v.p, d.p, e->ctx->stream));
  TRY(d.get(items, n * p->item_size, e->ctx->stream));
  HIPCHK(hipStreamSynchronize(e->ctx->stream));
  return EG_OK;
}
// ActiveParticipant::decrypt_share per item, with the radix-16 table of each R in the engine's generator workspace
static int share_prove_device(eg_proof_params* p, const uint8_t secret_share[32], uint64_t base_seed, size_t first, size_t n,
                              uint64_t rng_skip, const void* d_ct_random, void* d_items, void* d_ok, hipStream_t s) {
  Engine* e = p->eng;
  HIPCHK(hipSetDevice(e->ctx->device));
  if (n == 0) return EG_OK;
  u32 sk[8], key[8];
  memcpy(sk, secret_share, 32);
  memcpy(key, e->key_bytes, 32);
  int blocks = 0;
  TRY(gen_workspace(e, n, egplan::gen_share_ws_words(), &blocks));
  eg_launch_share_prove(blocks, s, base_seed + first, n, rng_skip, sk, key, reinterpret_cast<const u32*>(d_ct_random), e->ctx->tabG,
                        e->d_prefixes, e->plan.gen_pre_logeq, reinterpret_cast<u32*>(d_items), reinterpret_cast<unsigned char*>(d_ok),
                        e->gen_ws);
  HIPCHK(hipGetLastError());
  return EG_OK;
}
int eg_share_prove_batch_device(eg_proof_params* p, const uint8_t secret_share[32], uint64_t base_seed, size_t first, size_t n,
                                uint64_t rng_skip, const void* d_ct_random, void* d_items, void* d_ok, void* stream) { EG_LOCK_P(p);
  if (!p || !secret_share || (n && (!d_ct_random || !d_items || !d_ok))) return fail(EG_ERR_BAD_ARG, "bad argument");
  if (p->kind != EG_PROOF_SHARE) return fail(EG_ERR_BAD_ARG, "not a decryption-share params object");
  return share_prove_device(p, secret_share, base_seed, first, n, rng_skip, d_ct_random, d_items, d_ok, (hipStream_t)stream);
}
int eg_share_prove_batch(eg_proof_params* p, const uint8_t secret_share[32], uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip,
                         const uint8_t* ct_random, uint8_t* items, uint8_t* ok) { EG_LOCK_P(p);
  if (!p || !secret_share || (n && (!ct_random || !items || !ok))) return fail(EG_ERR_BAD_ARG, "bad argument");
  if (p->kind != EG_PROOF_SHARE) return fail(EG_ERR_BAD_ARG, "not a decryption-share params object");
  if (!eghost::scalar_bytes_canonical(secret_share)) return fail(EG_ERR_BAD_ARG, "the secret share is not a canonical scalar");
  Engine* e = p->eng;
  HIPCHK(hipSetDevice(e->ctx->device));
  DevBuf r, d, o;
  TRY(r.alloc(n * 32)); TRY(d.alloc(n * 128)); TRY(o.alloc(n));
  TRY(r.put(ct_random, n * 32, e->ctx->stream));
  TRY(share_prove_device(p, secret_share, base_seed, first, n, rng_skip, r.p, d.p, o.p, e->ctx->stream));
  TRY(d.get(items, n * 128, e->ctx->stream));
  TRY(o.get(ok, n, e->ctx->stream));
  HIPCHK(hipStreamSynchronize(e->ctx->stream));
  return EG_OK;
}

// ---- Merlin transcripts as a primitive (merlin 3.0.0 via src/proofs/mod.rs:39-57): known-answer tests on the device ----------
int eg_merlin_challenge_batch(eg_ctx* c, size_t n, const char* proto, size_t proto_len, const char* msg_label, size_t msg_label_len,
                              const uint8_t* msgs, size_t msg_len, const char* chal_label, size_t chal_label_len, uint8_t* out,
                              size_t out_len) { EG_LOCK(c);
  if (!c || !proto || !msg_label || !chal_label || (n && (!out || (msg_len && !msgs)))) return fail(EG_ERR_BAD_ARG, "bad argument");
  if (proto_len > 255 || msg_label_len > 255 || chal_label_len > 255 || out_len == 0 || out_len > 1024 || msg_len > (1u << 20))
    return fail(EG_ERR_BAD_ARG, "labels up to 255 bytes, challenges of 1..1024 bytes, messages up to 1 MiB");
  if (n == 0) return EG_OK;
  HIPCHK(hipSetDevice(c->device));
  std::vector<uint8_t> labels;
  labels.insert(labels.end(), proto, proto + proto_len);
  labels.insert(labels.end(), msg_label, msg_label + msg_label_len);
  labels.insert(labels.end(), chal_label, chal_label + chal_label_len);
  DevBuf l, m, o;
  TRY(l.alloc(labels.size())); TRY(m.alloc(n * msg_len)); TRY(o.alloc(n * out_len));
  TRY(l.put(labels.data(), labels.size(), c->stream)); TRY(m.put(msgs, n * msg_len, c->stream));
  hipLaunchKernelGGL(k_prim_merlin, dim3(blocks_of(n)), dim3(NT), 0, c->stream, n, (const unsigned char*)l.p, (int)proto_len,
                     (int)msg_label_len, (int)chal_label_len, (const unsigned char*)m.p, (int)msg_len, (unsigned char*)o.p, (int)out_len);
  TRY(o.get(out, n * out_len, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipGetLastError());
  return EG_OK;
}

// ---- voter signatures: Ed25519 of a batch (ed25519_kernels.cuh; the rule: include/eg_hip.h) -------------------------------------------
// Stateless like weeding: the generator's comb is immutable once the context exists, everything else is the caller's - no lock, no
// workspace of the context.
// The argument rules come first and need no context (so they can be tested without a GPU); what passes them fails on a null context.
static int ed_check_messages(size_t n, const void* msgs, size_t msg_stride, size_t msg_len, const void* prefix, size_t prefix_len) {
  if (const char* why = eged::refuse_messages(n, msgs != nullptr, msg_stride, msg_len, prefix != nullptr, prefix_len))
    return fail(EG_ERR_BAD_ARG, std::string("ed25519: ") + why);
  return EG_OK;
}
static int ed_check_roster(size_t n, const void* keys, size_t n_keys, const void* key_index, const void* sigs, const void* status_out) {
  if (n && (!keys || !sigs || !status_out)) return fail(EG_ERR_BAD_ARG, "ed25519: null keys, sigs or status_out");
  if (const char* why = eged::refuse_roster(n, n_keys, key_index != nullptr)) return fail(EG_ERR_BAD_ARG, std::string("ed25519: ") + why);
  return EG_OK;
}
size_t eg_ed25519_verify_scratch_bytes(const eg_ctx* c, size_t n) {
  return c && n < eged::N_LIMIT ? eged::layout(n, (unsigned)c->cus).total : 0;
}
int eg_ed25519_verify_device(eg_ctx* c, size_t n, const void* d_msgs, size_t msg_stride, size_t msg_len, const uint8_t* prefix, size_t prefix_len,
                             const void* d_keys, size_t n_keys, const void* d_key_index, const void* d_sigs, const void* d_status_in,
                             void* d_status_out, void* d_scratch, size_t scratch_bytes, void* stream) {
  TRY_(ed_check_messages(n, d_msgs, msg_stride, msg_len, prefix, prefix_len));
  TRY_(ed_check_roster(n, d_keys, n_keys, d_key_index, d_sigs, d_status_out));
  if (((uintptr_t)d_keys | (uintptr_t)d_sigs | (uintptr_t)d_key_index | (uintptr_t)d_status_in | (uintptr_t)d_status_out) & 3u)
    return fail(EG_ERR_BAD_ARG, "ed25519: keys, sigs, key_index and the status arrays must be 4-byte aligned");
  TRY_(check_ctx("ed25519", c));
  if (n == 0) return EG_OK;
  const eged::Layout L = eged::layout(n, (unsigned)c->cus);
  if (!d_scratch || scratch_bytes < L.total) return fail(EG_ERR_BAD_ARG, "ed25519: scratch is null or too small (eg_ed25519_verify_scratch_bytes says how much)");
  if ((uintptr_t)d_scratch & 15u) return fail(EG_ERR_BAD_ARG, "ed25519: scratch must be 16-byte aligned");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  char* base = static_cast<char*>(d_scratch);
  if (prefix_len) HIPCHK(hipMemcpyAsync(base + L.prefix, prefix, prefix_len, hipMemcpyHostToDevice, s));
  const EdItems it{static_cast<const unsigned char*>(d_msgs), msg_stride, msg_len, reinterpret_cast<const unsigned char*>(base + L.prefix), prefix_len};
  const EdRoster ro{static_cast<const u32*>(d_keys), n_keys, static_cast<const u32*>(d_key_index)};
  u32* h = reinterpret_cast<u32*>(base + L.h);
  hipLaunchKernelGGL(k_ed25519_hash, dim3(blocks_of(n)), dim3(NT), 0, s, n, it, ro, static_cast<const u32*>(d_sigs), static_cast<const u32*>(d_status_in), h);
  hipLaunchKernelGGL(k_ed25519_verify, dim3(L.blocks), dim3(NT), 0, s, n, ro, static_cast<const u32*>(d_sigs), (const u32*)h,
                     static_cast<const u32*>(d_status_in), static_cast<u32*>(d_status_out), (const uint4*)c->tabG,
                     reinterpret_cast<uint4*>(base + L.tables));
  HIPCHK(hipGetLastError());
  return EG_OK;
}
static size_t ed_msgs_bytes(size_t n, size_t msg_stride, size_t msg_len) { return n ? (n - 1) * msg_stride + msg_len : 0; }
int eg_ed25519_verify_batch(eg_ctx* c, size_t n, const uint8_t* msgs, size_t msg_stride, size_t msg_len, const uint8_t* prefix, size_t prefix_len,
                            const uint8_t* keys, size_t n_keys, const uint32_t* key_index, const uint8_t* sigs, const uint32_t* status_in,
                            uint32_t* status_out) {
  TRY_(ed_check_messages(n, msgs, msg_stride, msg_len, prefix, prefix_len));
  TRY_(ed_check_roster(n, keys, n_keys, key_index, sigs, status_out));
  TRY_(check_ctx("ed25519", c));
  if (n == 0) return EG_OK;
  HIPCHK(hipSetDevice(c->device));
  HostStage st("ed25519"); TRY_(st.open());
  const size_t need = eg_ed25519_verify_scratch_bytes(c, n);
  void *dm, *dk, *di = nullptr, *ds, *dsi = nullptr, *dso, *scratch;
  TRY_(st.put(&dm, msgs, ed_msgs_bytes(n, msg_stride, msg_len)));
  TRY_(st.put(&dk, keys, n_keys * 32));
  if (key_index) TRY_(st.put(&di, key_index, n * 4));
  TRY_(st.put(&ds, sigs, n * 64));
  if (status_in) TRY_(st.put(&dsi, status_in, n * 4));
  TRY_(st.put(&dso, nullptr, n * 4));
  TRY_(st.put(&scratch, nullptr, need));
  TRY_(eg_ed25519_verify_device(c, n, dm, msg_stride, msg_len, prefix, prefix_len, dk, n_keys, di, ds, dsi, dso, scratch, need, st.s));
  TRY_(st.get(status_out, dso, n * 4));
  TRY_(st.sync());
  return EG_OK;
}
int eg_ed25519_keypair_batch_device(eg_ctx* c, size_t n, const void* d_seeds, void* d_keys, void* stream) {
  if (n >= eged::N_LIMIT) return fail(EG_ERR_BAD_ARG, "ed25519: n is 2^31 or more");
  if ((n && (!d_seeds || !d_keys)) || ((uintptr_t)d_keys & 3u)) return fail(EG_ERR_BAD_ARG, "ed25519: null seeds or keys, or keys not 4-byte aligned");
  TRY_(check_ctx("ed25519", c));
  if (n == 0) return EG_OK;
  HIPCHK(hipSetDevice(c->device));
  hipLaunchKernelGGL(k_ed25519_keypair, dim3(blocks_of(n)), dim3(NT), 0, (hipStream_t)stream, n, static_cast<const unsigned char*>(d_seeds),
                     (const uint4*)c->tabG, static_cast<u32*>(d_keys));
  HIPCHK(hipGetLastError());
  return EG_OK;
}
int eg_ed25519_keypair_batch(eg_ctx* c, size_t n, const uint8_t* seeds, uint8_t* keys) {
  if (n >= eged::N_LIMIT) return fail(EG_ERR_BAD_ARG, "ed25519: n is 2^31 or more");
  if (n && (!seeds || !keys)) return fail(EG_ERR_BAD_ARG, "ed25519: null seeds or keys");
  TRY_(check_ctx("ed25519", c));
  if (n == 0) return EG_OK;
  HIPCHK(hipSetDevice(c->device));
  HostStage st("ed25519"); TRY_(st.open());
  void *dse, *dk;
  TRY_(st.put(&dse, seeds, n * 32)); TRY_(st.put(&dk, nullptr, n * 32));
  TRY_(eg_ed25519_keypair_batch_device(c, n, dse, dk, st.s));
  TRY_(st.get(keys, dk, n * 32));
  TRY_(st.sync());
  return EG_OK;
}
int eg_ed25519_sign_batch_device(eg_ctx* c, size_t n, const void* d_seeds, const void* d_msgs, size_t msg_stride, size_t msg_len,
                                 const void* d_prefix, size_t prefix_len, void* d_sigs, void* stream) {
  TRY_(ed_check_messages(n, d_msgs, msg_stride, msg_len, d_prefix, prefix_len));
  if ((n && (!d_seeds || !d_sigs)) || ((uintptr_t)d_sigs & 3u)) return fail(EG_ERR_BAD_ARG, "ed25519: null seeds or sigs, or sigs not 4-byte aligned");
  TRY_(check_ctx("ed25519", c));
  if (n == 0) return EG_OK;
  HIPCHK(hipSetDevice(c->device));
  const EdItems it{static_cast<const unsigned char*>(d_msgs), msg_stride, msg_len, static_cast<const unsigned char*>(d_prefix), prefix_len};
  hipLaunchKernelGGL(k_ed25519_sign, dim3(blocks_of(n)), dim3(NT), 0, (hipStream_t)stream, n, static_cast<const unsigned char*>(d_seeds), it,
                     (const uint4*)c->tabG, static_cast<u32*>(d_sigs));
  HIPCHK(hipGetLastError());
  return EG_OK;
}
int eg_ed25519_sign_batch(eg_ctx* c, size_t n, const uint8_t* seeds, const uint8_t* msgs, size_t msg_stride, size_t msg_len, const uint8_t* prefix,
                          size_t prefix_len, uint8_t* sigs) {
  TRY_(ed_check_messages(n, msgs, msg_stride, msg_len, prefix, prefix_len));
  if (n && (!seeds || !sigs)) return fail(EG_ERR_BAD_ARG, "ed25519: null seeds or sigs");
  TRY_(check_ctx("ed25519", c));
  if (n == 0) return EG_OK;
  HIPCHK(hipSetDevice(c->device));
  HostStage st("ed25519"); TRY_(st.open());
  void *dse, *dm, *dp, *dsg;
  TRY_(st.put(&dse, seeds, n * 32)); TRY_(st.put(&dm, msgs, ed_msgs_bytes(n, msg_stride, msg_len)));
  TRY_(st.put(&dp, prefix, prefix_len)); TRY_(st.put(&dsg, nullptr, n * 64));
  TRY_(eg_ed25519_sign_batch_device(c, n, dse, dm, msg_stride, msg_len, dp, prefix_len, dsg, st.s));
  TRY_(st.get(sigs, dsg, n * 64));
  TRY_(st.sync());
  return EG_OK;
}
int eg_sha512_batch_device(eg_ctx* c, size_t n, const void* d_msgs, size_t msg_stride, size_t msg_len, const void* d_prefix, size_t prefix_len,
                           void* d_digests, void* stream) {
  TRY_(ed_check_messages(n, d_msgs, msg_stride, msg_len, d_prefix, prefix_len));
  if ((n && !d_digests) || ((uintptr_t)d_digests & 3u)) return fail(EG_ERR_BAD_ARG, "sha512: digests null or not 4-byte aligned");
  TRY_(check_ctx("ed25519", c));
  if (n == 0) return EG_OK;
  HIPCHK(hipSetDevice(c->device));
  const EdItems it{static_cast<const unsigned char*>(d_msgs), msg_stride, msg_len, static_cast<const unsigned char*>(d_prefix), prefix_len};
  hipLaunchKernelGGL(k_sha512, dim3(blocks_of(n)), dim3(NT), 0, (hipStream_t)stream, n, it, static_cast<u32*>(d_digests));
  HIPCHK(hipGetLastError());
  return EG_OK;
}
int eg_sha512_batch(eg_ctx* c, size_t n, const uint8_t* msgs, size_t msg_stride, size_t msg_len, const uint8_t* prefix, size_t prefix_len,
                    uint8_t* digests) {
  TRY_(ed_check_messages(n, msgs, msg_stride, msg_len, prefix, prefix_len));
  if (n && !digests) return fail(EG_ERR_BAD_ARG, "sha512: null digests");
  TRY_(check_ctx("ed25519", c));
  if (n == 0) return EG_OK;
  HIPCHK(hipSetDevice(c->device));
  HostStage st("ed25519"); TRY_(st.open());
  void *dm, *dp, *dd;
  TRY_(st.put(&dm, msgs, ed_msgs_bytes(n, msg_stride, msg_len))); TRY_(st.put(&dp, prefix, prefix_len)); TRY_(st.put(&dd, nullptr, n * 64));
  TRY_(eg_sha512_batch_device(c, n, dm, msg_stride, msg_len, dp, prefix_len, dd, st.s));
  TRY_(st.get(digests, dd, n * 64));
  TRY_(st.sync());
  return EG_OK;
}

// ---- voter roll: the one ballot of every voter that counts (roll_kernels.cuh; the rule: include/eg_hip.h) -------------------------------
// Stateless like weeding and the signature pass: everything is the caller's - no lock, no workspace of the context.
// The argument rules come first and need no context (so they can be tested without a GPU); what passes them fails on a null context.
static int roll_check_args(size_t n, size_t n_keys, uint64_t seq_base, int policy, const egr::Have& h) {
  if (const char* why = egr::refuse(n, n_keys, seq_base, policy, h)) return fail(EG_ERR_BAD_ARG, std::string("roll: ") + why);
  return EG_OK;
}
static const AlignedMsgs ROLL_ALIGNED{"roll: roll, roster_weights, superseded_by, weights_out, displaced and displaced_count must be 8-byte aligned",
                                      "roll: key_index, the status arrays, roster_groups, groups_out, found and scratch must be 4-byte aligned"};
size_t eg_roll_cast_scratch_bytes(const eg_ctx* c, size_t n, size_t n_keys) {
  return c && !egr::refuse_sizes(n, n_keys) ? egr::layout(n, n_keys).total : 0;
}
int eg_roll_cast_device(eg_ctx* c, size_t n, const void* d_key_index, const void* d_status_in, uint64_t seq_base, int policy, void* d_roll,
                        size_t n_keys, const void* d_roster_groups, const void* d_roster_weights, void* d_superseded_by, void* d_status_out,
                        void* d_groups_out, void* d_weights_out, void* d_displaced, void* d_displaced_count, void* d_found, void* d_scratch,
                        size_t scratch_bytes, void* stream) {
  TRY_(roll_check_args(n, n_keys, seq_base, policy,
                       egr::Have{d_key_index != nullptr, d_roll != nullptr, d_superseded_by != nullptr, d_found != nullptr, d_roster_groups != nullptr,
                                 d_roster_weights != nullptr, d_groups_out != nullptr, d_weights_out != nullptr, d_displaced != nullptr,
                                 d_displaced_count != nullptr}));
  TRY_(check_aligned(ROLL_ALIGNED,
                     (uintptr_t)d_roll | (uintptr_t)d_roster_weights | (uintptr_t)d_superseded_by | (uintptr_t)d_weights_out |
                         (uintptr_t)d_displaced | (uintptr_t)d_displaced_count,
                     (uintptr_t)d_key_index | (uintptr_t)d_status_in | (uintptr_t)d_status_out | (uintptr_t)d_roster_groups |
                         (uintptr_t)d_groups_out | (uintptr_t)d_found | (uintptr_t)d_scratch));
  const egr::Layout L = egr::layout(n, n_keys);
  if (L.total && (!d_scratch || scratch_bytes < L.total))
    return fail(EG_ERR_BAD_ARG, "roll: scratch is null or too small (eg_roll_cast_scratch_bytes says how much)");
  TRY_(check_ctx("roll", c));
  if (!d_found && !d_displaced_count) return EG_OK;                       // n == 0 and nowhere to write anything to
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  u32* found = static_cast<u32*>(d_found);
  if (found) HIPCHK(hipMemsetAsync(found, 0, 3 * sizeof(u32), s));
  if (n == 0) {
    if (d_displaced_count) HIPCHK(hipMemsetAsync(d_displaced_count, 0, sizeof(uint64_t), s));
    return EG_OK;
  }
  char* base = static_cast<char*>(d_scratch);
  u32* best = reinterpret_cast<u32*>(base + L.best);
  u32* flag = reinterpret_cast<u32*>(base + L.flag);
  u32* tiles = reinterpret_cast<u32*>(base + L.tiles);
  const u32* status = static_cast<const u32*>(d_status_in);
  const RollMemDev mem{static_cast<const u32*>(d_key_index), best, static_cast<unsigned long long*>(d_roll), static_cast<const u32*>(d_roster_groups),
                       static_cast<const unsigned long long*>(d_roster_weights), static_cast<unsigned long long*>(d_displaced)};
  const RollOutDev out{static_cast<unsigned long long*>(d_superseded_by), static_cast<u32*>(d_status_out), static_cast<u32*>(d_groups_out),
                       static_cast<unsigned long long*>(d_weights_out)};
  const unsigned blocks = (unsigned)((n + ROLL_NT - 1) / ROLL_NT);
  HIPCHK(hipMemsetAsync(best, 0, n_keys * sizeof(u32), s));
  hipLaunchKernelGGL(k_roll_claim, dim3(blocks), dim3(ROLL_NT), 0, s, mem, status, (uint64_t)n, policy, (uint64_t)n_keys);
  hipLaunchKernelGGL(k_roll_resolve, dim3(blocks), dim3(ROLL_NT), 0, s, mem, status, (uint64_t)n, seq_base, policy, (uint64_t)n_keys, out, flag, found);
  if (d_displaced) {
    hipLaunchKernelGGL(k_roll_scan_tiles, dim3(L.n_tiles), dim3(ROLL_NT), 0, s, (const u32*)flag, (u32)n, tiles);
    hipLaunchKernelGGL(k_roll_scan_tops, dim3(1), dim3(64), 0, s, L.n_tiles, tiles, static_cast<unsigned long long*>(d_displaced_count));
    hipLaunchKernelGGL(k_roll_scan_apply, dim3(L.n_tiles), dim3(ROLL_NT), 0, s, flag, (u32)n, (const u32*)tiles);
  }
  hipLaunchKernelGGL(k_roll_commit, dim3(blocks), dim3(ROLL_NT), 0, s, mem, (const u32*)flag, (uint64_t)n, seq_base, policy, (uint64_t)n_keys);
  HIPCHK(hipGetLastError());
  return EG_OK;
}
int eg_roll_check_device(eg_ctx* c, size_t n, const void* d_key_index, const void* d_status_in, uint64_t seq_base, int policy, const void* d_roll,
                         size_t n_keys, const void* d_roster_groups, const void* d_roster_weights, void* d_superseded_by, void* d_status_out,
                         void* d_groups_out, void* d_weights_out, void* d_found, void* stream) {
  TRY_(roll_check_args(n, n_keys, seq_base, policy,
                       egr::Have{d_key_index != nullptr, d_roll != nullptr, d_superseded_by != nullptr, d_found != nullptr, d_roster_groups != nullptr,
                                 d_roster_weights != nullptr, d_groups_out != nullptr, d_weights_out != nullptr, false, false}));
  TRY_(check_aligned(ROLL_ALIGNED, (uintptr_t)d_roll | (uintptr_t)d_roster_weights | (uintptr_t)d_superseded_by | (uintptr_t)d_weights_out,
                     (uintptr_t)d_key_index | (uintptr_t)d_status_in | (uintptr_t)d_status_out | (uintptr_t)d_roster_groups |
                         (uintptr_t)d_groups_out | (uintptr_t)d_found));
  TRY_(check_ctx("roll", c));
  if (!d_found) return EG_OK;                                             // n == 0 and nowhere to write anything to
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  u32* found = static_cast<u32*>(d_found);
  HIPCHK(hipMemsetAsync(found, 0, 3 * sizeof(u32), s));
  if (n == 0) return EG_OK;
  // the roll is only read: the lane function has no store, the cast away of const serves the shared view of the memory
  const RollMemDev mem{static_cast<const u32*>(d_key_index), nullptr, static_cast<unsigned long long*>(const_cast<void*>(d_roll)),
                       static_cast<const u32*>(d_roster_groups), static_cast<const unsigned long long*>(d_roster_weights), nullptr};
  const RollOutDev out{static_cast<unsigned long long*>(d_superseded_by), static_cast<u32*>(d_status_out), static_cast<u32*>(d_groups_out),
                       static_cast<unsigned long long*>(d_weights_out)};
  hipLaunchKernelGGL(k_roll_check, dim3((unsigned)((n + ROLL_NT - 1) / ROLL_NT)), dim3(ROLL_NT), 0, s, mem, static_cast<const u32*>(d_status_in),
                     (uint64_t)n, seq_base, policy, (uint64_t)n_keys, out, found);
  HIPCHK(hipGetLastError());
  return EG_OK;
}
// host arrays, staged on a stream of the call's own; `cast`: the roll comes back, with the displaced entries
static int roll_host(eg_ctx* c, bool cast, size_t n, const uint32_t* key_index, const uint32_t* status_in, uint64_t seq_base, int policy,
                     const uint64_t* roll, uint64_t* roll_out, size_t n_keys, const uint32_t* roster_groups, const uint64_t* roster_weights,
                     uint64_t* superseded_by, uint32_t* status_out, uint32_t* groups_out, uint64_t* weights_out, uint64_t* displaced,
                     uint64_t* displaced_count, uint32_t* found) {
  TRY_(roll_check_args(n, n_keys, seq_base, policy,
                       egr::Have{key_index != nullptr, roll != nullptr, superseded_by != nullptr, found != nullptr, roster_groups != nullptr,
                                 roster_weights != nullptr, groups_out != nullptr, weights_out != nullptr, displaced != nullptr,
                                 displaced_count != nullptr}));
  TRY_(check_ctx("roll", c));
  if (found) found[0] = found[1] = found[2] = 0;
  if (displaced_count) *displaced_count = 0;
  if (n == 0) return EG_OK;
  HIPCHK(hipSetDevice(c->device));
  HostStage st("roll"); TRY_(st.open());
  const size_t need = cast ? eg_roll_cast_scratch_bytes(c, n, n_keys) : 0;
  void *di, *dsi = nullptr, *dr, *dg = nullptr, *dw = nullptr, *dby, *dso = nullptr, *dgo = nullptr, *dwo = nullptr, *dd = nullptr, *dtail, *scratch = nullptr;
  TRY_(st.put(&di, key_index, n * 4));
  if (status_in) TRY_(st.put(&dsi, status_in, n * 4));
  TRY_(st.put(&dr, roll, n_keys * 8));
  if (roster_groups) TRY_(st.put(&dg, roster_groups, n_keys * 4));
  if (roster_weights) TRY_(st.put(&dw, roster_weights, n_keys * 8));
  TRY_(st.put(&dby, nullptr, n * 8));
  if (status_out) TRY_(st.put(&dso, nullptr, n * 4));
  if (groups_out) TRY_(st.put(&dgo, nullptr, n * 4));
  if (weights_out) TRY_(st.put(&dwo, nullptr, n * 8));
  if (displaced) TRY_(st.put(&dd, nullptr, n * 16));
  TRY_(st.put(&dtail, nullptr, 32));                                      // the displaced count (uint64), then the three counters
  if (cast) TRY_(st.put(&scratch, nullptr, need));
  void* d_count = displaced ? dtail : nullptr;
  void* d_found = static_cast<char*>(dtail) + 8;
  if (cast)
    TRY_(eg_roll_cast_device(c, n, di, dsi, seq_base, policy, dr, n_keys, dg, dw, dby, dso, dgo, dwo, dd, d_count, d_found, scratch, need, st.s));
  else
    TRY_(eg_roll_check_device(c, n, di, dsi, seq_base, policy, dr, n_keys, dg, dw, dby, dso, dgo, dwo, d_found, st.s));
  unsigned long long count = 0;
  TRY_(st.get(superseded_by, dby, n * 8));
  if (status_out) TRY_(st.get(status_out, dso, n * 4));
  if (groups_out) TRY_(st.get(groups_out, dgo, n * 4));
  if (weights_out) TRY_(st.get(weights_out, dwo, n * 8));
  if (cast) TRY_(st.get(roll_out, dr, n_keys * 8));
  TRY_(st.get(found, d_found, 3 * sizeof(u32)));
  if (displaced) TRY_(st.get(&count, d_count, sizeof count));
  TRY_(st.sync());
  if (displaced && count && count <= n) {
    TRY_(st.get(displaced, dd, (size_t)count * 16));
    TRY_(st.sync());
  }
  if (displaced_count) *displaced_count = count;
  return EG_OK;
}
int eg_roll_cast(eg_ctx* c, size_t n, const uint32_t* key_index, const uint32_t* status_in, uint64_t seq_base, int policy, uint64_t* roll,
                 size_t n_keys, const uint32_t* roster_groups, const uint64_t* roster_weights, uint64_t* superseded_by, uint32_t* status_out,
                 uint32_t* groups_out, uint64_t* weights_out, uint64_t* displaced, uint64_t* displaced_count, uint32_t* found) {
  return roll_host(c, true, n, key_index, status_in, seq_base, policy, roll, roll, n_keys, roster_groups, roster_weights, superseded_by, status_out,
                   groups_out, weights_out, displaced, displaced_count, found);
}
int eg_roll_check(eg_ctx* c, size_t n, const uint32_t* key_index, const uint32_t* status_in, uint64_t seq_base, int policy, const uint64_t* roll,
                  size_t n_keys, const uint32_t* roster_groups, const uint64_t* roster_weights, uint64_t* superseded_by, uint32_t* status_out,
                  uint32_t* groups_out, uint64_t* weights_out, uint32_t* found) {
  return roll_host(c, false, n, key_index, status_in, seq_base, policy, roll, nullptr, n_keys, roster_groups, roster_weights, superseded_by,
                   status_out, groups_out, weights_out, nullptr, nullptr, found);
}

// ---- receipt log: leaf hashes, the Merkle tree above them, audit paths and their check (merkle_kernels.cuh; the rule: include/eg_hip.h) ----
// Stateless like weeding and the roll: everything is the caller's - no lock, no workspace of the context, no allocation, no synchronisation
// in the _device forms.  The argument rules come first and need no context (so they can be tested without a GPU); what passes them fails on
// a null context.
static int merkle_refuse(const char* why) { return why ? fail(EG_ERR_BAD_ARG, std::string("merkle: ") + why) : EG_OK; }
static const AlignedMsgs MERKLE_ALIGNED{"merkle: leaf_index, log_count and index must be 8-byte aligned",
                                        "merkle: leaves, log, nodes, paths, root, path_len, verdict, the status words, found and scratch must be 4-byte aligned"};
int eg_merkle_depth(uint64_t n_leaves) { return egm::depth(n_leaves); }
size_t eg_merkle_nodes_bytes(uint64_t n_leaves) { return n_leaves < egm::LEAVES_MAX ? (size_t)egm::nodes_total(n_leaves) * egm::HASH_BYTES : 0; }
int eg_merkle_level(uint64_t n_leaves, int level, uint64_t* offset, uint64_t* count) {
  if (n_leaves >= egm::LEAVES_MAX) return merkle_refuse("N is 2^31 or more");
  if (level < 0 || level > egm::depth(n_leaves)) return merkle_refuse("level is not in 0 .. depth(N)");
  if (!offset || !count) return merkle_refuse("null offset or count");
  *offset = level ? egm::level_offset(n_leaves, level) * egm::HASH_BYTES : 0u;
  *count = egm::level_count(n_leaves, level);
  return EG_OK;
}
size_t eg_merkle_leaves_scratch_bytes(size_t n) { return n < egm::LEAVES_MAX ? egm::leaf_layout(n).total : 0; }
size_t eg_merkle_tree_scratch_bytes(uint64_t n_leaves) { return n_leaves < egm::LEAVES_MAX ? egm::tree_layout(n_leaves).total : 0; }

// the launches of the leaf pass; `tail` = entry n_prior of the log with room for `room` entries, or null: no append
static int merkle_leaves_run(eg_ctx* c, size_t n, MerkleItems it, const uint8_t* prefix, size_t prefix_len, const u32* status, uint64_t n_prior,
                             void* d_leaf_index, void* d_leaves_out, u32* tail, uint64_t room, void* d_log_count, void* d_found, void* d_scratch,
                             hipStream_t s) {
  HIPCHK(hipSetDevice(c->device));
  u32* found = static_cast<u32*>(d_found);
  unsigned long long* count = static_cast<unsigned long long*>(d_log_count);
  if (n == 0) {                                                         // no leaves: the count is n_prior, the found words are zero
    if (found || count) hipLaunchKernelGGL(k_merkle_scan_tops, dim3(1), dim3(64), 0, s, 0u, (u32*)nullptr, n_prior, room, (u32*)nullptr, count, found);
    HIPCHK(hipGetLastError());
    return EG_OK;
  }
  const egm::LeafLayout L = egm::leaf_layout(n);
  char* base = static_cast<char*>(d_scratch);
  unsigned char* head = reinterpret_cast<unsigned char*>(base + L.head);
  u32* pos = reinterpret_cast<u32*>(base + L.pos);
  u32* tiles = reinterpret_cast<u32*>(base + L.tiles);
  u32* total_word = reinterpret_cast<u32*>(base + L.total_word);
  u32* rows = d_leaves_out ? static_cast<u32*>(d_leaves_out) : reinterpret_cast<u32*>(base + L.leaves);
  HIPCHK(hipMemsetAsync(head, 0, 1, s));                                // the domain byte of a leaf
  if (prefix_len) HIPCHK(hipMemcpyAsync(head + 1, prefix, prefix_len, hipMemcpyHostToDevice, s));
  it.head = head;
  it.head_len = 1 + prefix_len;
  const MerkleLeafDev leaf{it, rows, d_leaves_out != nullptr, pos};
  const MerklePlaceDev place{pos, rows, static_cast<unsigned long long*>(d_leaf_index), tail};
  hipLaunchKernelGGL(k_merkle_leaf, dim3((unsigned)((n + MERKLE_NT - 1) / MERKLE_NT)), dim3(MERKLE_NT), 0, s, leaf, status, (uint64_t)n);
  hipLaunchKernelGGL(k_merkle_scan_tiles, dim3(L.n_tiles), dim3(MERKLE_NT), 0, s, (const u32*)pos, (u32)n, tiles);
  hipLaunchKernelGGL(k_merkle_scan_tops, dim3(1), dim3(64), 0, s, L.n_tiles, tiles, n_prior, room, total_word, count, found);
  hipLaunchKernelGGL(k_merkle_scan_apply, dim3(L.n_tiles), dim3(MERKLE_NT), 0, s, pos, (u32)n, (const u32*)tiles);
  hipLaunchKernelGGL(k_merkle_place, dim3((unsigned)((n * 8 + MERKLE_NT - 1) / MERKLE_NT)), dim3(MERKLE_NT), 0, s, place, (uint64_t)n, n_prior, room,
                     (const u32*)total_word);
  HIPCHK(hipGetLastError());
  return EG_OK;
}
int eg_merkle_leaves_device(eg_ctx* c, size_t n, const void* d_msgs, size_t msg_stride, size_t msg_len, const uint8_t* prefix, size_t prefix_len,
                            const void* d_extra, size_t extra_stride, size_t extra_len, const void* d_status_in, uint64_t n_prior,
                            void* d_leaf_index, void* d_leaves_out, void* d_log, uint64_t log_cap, void* d_log_count, void* d_found,
                            void* d_scratch, size_t scratch_bytes, void* stream) {
  TRY_(merkle_refuse(egm::refuse_messages(n, d_msgs != nullptr, msg_stride, msg_len, prefix != nullptr, prefix_len, d_extra != nullptr, extra_stride,
                                          extra_len)));
  TRY_(merkle_refuse(egm::refuse_leaves(n, n_prior, d_leaf_index != nullptr, d_found != nullptr, d_log != nullptr, d_log_count != nullptr, log_cap)));
  TRY_(check_aligned(MERKLE_ALIGNED, (uintptr_t)d_leaf_index | (uintptr_t)d_log_count,
                     (uintptr_t)d_leaves_out | (uintptr_t)d_log | (uintptr_t)d_status_in | (uintptr_t)d_found | (uintptr_t)d_scratch));
  const size_t need = egm::leaf_layout(n).total;
  if (need && (!d_scratch || scratch_bytes < need)) return merkle_refuse("scratch is null or too small (eg_merkle_leaves_scratch_bytes says how much)");
  TRY_(check_ctx("merkle", c));
  const MerkleItems it{static_cast<const unsigned char*>(d_msgs), msg_stride, msg_len, extra_len ? static_cast<const unsigned char*>(d_extra) : nullptr,
                       extra_stride, extra_len, nullptr, 0};
  u32* tail = d_log_count ? static_cast<u32*>(d_log) + n_prior * egm::HASH_WORDS : nullptr;
  return merkle_leaves_run(c, n, it, prefix, prefix_len, static_cast<const u32*>(d_status_in), n_prior, d_leaf_index, d_leaves_out, tail,
                           d_log_count ? log_cap - n_prior : 0u, d_log_count, d_found, d_scratch, (hipStream_t)stream);
}
int eg_merkle_leaves(eg_ctx* c, size_t n, const uint8_t* msgs, size_t msg_stride, size_t msg_len, const uint8_t* prefix, size_t prefix_len,
                     const uint8_t* extra, size_t extra_stride, size_t extra_len, const uint32_t* status_in, uint64_t n_prior, uint64_t* leaf_index,
                     uint8_t* leaves_out, uint8_t* log, uint64_t log_cap, uint64_t* log_count, uint32_t* found) {
  TRY_(merkle_refuse(egm::refuse_messages(n, msgs != nullptr, msg_stride, msg_len, prefix != nullptr, prefix_len, extra != nullptr, extra_stride, extra_len)));
  TRY_(merkle_refuse(egm::refuse_leaves(n, n_prior, leaf_index != nullptr, found != nullptr, log != nullptr, log_count != nullptr, log_cap)));
  TRY_(check_ctx("merkle", c));
  if (found) found[0] = found[1] = 0;
  if (log_count) *log_count = n_prior;
  if (n == 0) return EG_OK;
  HIPCHK(hipSetDevice(c->device));
  HostStage st("merkle"); TRY_(st.open());
  const size_t need = eg_merkle_leaves_scratch_bytes(n);
  const uint64_t room = log_count ? log_cap - n_prior : 0u;
  const size_t tail_rows = (size_t)std::min<uint64_t>(room, n);       // at most n leaves are appended, and never more than fit
  void *dm = nullptr, *de = nullptr, *dsi = nullptr, *di, *dl = nullptr, *dt = nullptr, *dtail, *scratch;
  if (msg_len) TRY_(st.put(&dm, msgs, ed_msgs_bytes(n, msg_stride, msg_len)));
  if (extra_len) TRY_(st.put(&de, extra, ed_msgs_bytes(n, extra_stride, extra_len)));
  if (status_in) TRY_(st.put(&dsi, status_in, n * 4));
  TRY_(st.put(&di, nullptr, n * 8));
  if (leaves_out) TRY_(st.put(&dl, nullptr, n * egm::HASH_BYTES));
  if (log_count) TRY_(st.put(&dt, nullptr, tail_rows * egm::HASH_BYTES));
  TRY_(st.put(&dtail, nullptr, 32));                                    // the count (uint64), then the two found words
  TRY_(st.put(&scratch, nullptr, need));
  void* d_count = log_count ? dtail : nullptr;
  void* d_found = static_cast<char*>(dtail) + 8;
  const MerkleItems it{static_cast<const unsigned char*>(dm), msg_stride, msg_len, static_cast<const unsigned char*>(de), extra_stride, extra_len, nullptr, 0};
  TRY_(merkle_leaves_run(c, n, it, prefix, prefix_len, static_cast<const u32*>(dsi), n_prior, di, dl, static_cast<u32*>(dt), room, d_count, d_found,
                         scratch, st.s));
  unsigned long long count = n_prior;
  TRY_(st.get(leaf_index, di, n * 8));
  if (leaves_out) TRY_(st.get(leaves_out, dl, n * egm::HASH_BYTES));
  TRY_(st.get(found, d_found, 2 * sizeof(u32)));
  if (log_count) TRY_(st.get(&count, d_count, sizeof count));
  TRY_(st.sync());
  if (log_count && count > n_prior && count - n_prior <= tail_rows) {
    TRY_(st.get(log + n_prior * egm::HASH_BYTES, dt, (size_t)(count - n_prior) * egm::HASH_BYTES));
    TRY_(st.sync());
  }
  if (log_count) *log_count = count;
  if (found[1]) return fail(EG_ERR_BAD_ARG, "merkle: the leaves do not fit the log (log_cap); nothing was appended");
  return EG_OK;
}

int eg_merkle_tree_device(eg_ctx* c, uint64_t n_leaves, const void* d_log, void* d_root, void* d_nodes, void* d_scratch, size_t scratch_bytes,
                          void* stream) {
  TRY_(merkle_refuse(egm::refuse_tree(n_leaves, d_log != nullptr, d_root != nullptr)));
  TRY_(check_aligned(MERKLE_ALIGNED, 0, (uintptr_t)d_log | (uintptr_t)d_root | (uintptr_t)d_nodes | (uintptr_t)d_scratch));
  const egm::TreeLayout L = egm::tree_layout(n_leaves);
  if (!d_nodes && L.total && (!d_scratch || scratch_bytes < L.total))
    return merkle_refuse("scratch is null or too small (eg_merkle_tree_scratch_bytes says how much a tree without a node store needs)");
  TRY_(check_ctx("merkle", c));
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  const u32* cur = static_cast<const u32*>(d_log);
  if (n_leaves == 0) cur = nullptr;
  char* base = static_cast<char*>(d_scratch);
  u32* store = static_cast<u32*>(d_nodes);
  const int depth = egm::depth(n_leaves);
  uint64_t n_in = n_leaves;
  bool pong = false;
  for (int level = 0; level < depth; pong = !pong) {
    MerkleTileArgs a;
    a.in = cur; a.n_in = n_in; a.store = store; a.steps = std::min(egm::T_LOG, depth - level);
    for (int k = 0; k < egm::T_LOG; ++k) a.off[k] = k < a.steps ? egm::level_offset(n_leaves, level + k + 1) : 0u;
    // without a store: the top level of the launch goes to the scratch, that of the last launch - one node - straight to the root
    const bool last = level + a.steps == depth;
    a.top = store ? nullptr : last ? static_cast<u32*>(d_root) : reinterpret_cast<u32*>(base + (pong ? L.pong : L.ping));
    const unsigned tiles = (unsigned)((n_in + (1u << egm::T_LOG) - 1) >> egm::T_LOG);
    hipLaunchKernelGGL(k_merkle_tile<egm::T_LOG>, dim3(tiles), dim3(1 << (egm::T_LOG - 2)), 0, s, a);
    cur = store ? store + a.off[a.steps - 1] * egm::HASH_WORDS : a.top;
    n_in = egm::level_count(n_in, a.steps);
    level += a.steps;
  }
  if (cur != static_cast<const u32*>(d_root)) hipLaunchKernelGGL(k_merkle_root, dim3(1), dim3(64), 0, s, cur, static_cast<u32*>(d_root));
  HIPCHK(hipGetLastError());
  return EG_OK;
}
int eg_merkle_tree(eg_ctx* c, uint64_t n_leaves, const uint8_t* log, uint8_t* root, uint8_t* nodes) {
  TRY_(merkle_refuse(egm::refuse_tree(n_leaves, log != nullptr, root != nullptr)));
  TRY_(check_ctx("merkle", c));
  HIPCHK(hipSetDevice(c->device));
  HostStage st("merkle"); TRY_(st.open());
  const size_t store_bytes = eg_merkle_nodes_bytes(n_leaves), need = nodes ? 0 : eg_merkle_tree_scratch_bytes(n_leaves);
  void *dl = nullptr, *dr, *dn = nullptr, *scratch = nullptr;
  if (n_leaves) TRY_(st.put(&dl, log, (size_t)n_leaves * egm::HASH_BYTES));
  TRY_(st.put(&dr, nullptr, egm::HASH_BYTES));
  if (nodes) TRY_(st.put(&dn, nullptr, store_bytes));
  if (need) TRY_(st.put(&scratch, nullptr, need));
  TRY_(eg_merkle_tree_device(c, n_leaves, dl, dr, dn, scratch, need, st.s));
  TRY_(st.get(root, dr, egm::HASH_BYTES));
  if (nodes && store_bytes) TRY_(st.get(nodes, dn, store_bytes));
  TRY_(st.sync());
  return EG_OK;
}

int eg_merkle_paths_device(eg_ctx* c, size_t m, const void* d_index, uint64_t n_leaves, const void* d_log, const void* d_nodes, void* d_paths,
                           void* d_path_len, void* stream) {
  TRY_(merkle_refuse(egm::refuse_paths(m, n_leaves, d_index != nullptr, d_log != nullptr, d_nodes != nullptr, d_paths != nullptr, d_path_len != nullptr)));
  TRY_(check_aligned(MERKLE_ALIGNED, (uintptr_t)d_index, (uintptr_t)d_log | (uintptr_t)d_nodes | (uintptr_t)d_paths | (uintptr_t)d_path_len));
  TRY_(check_ctx("merkle", c));
  if (m == 0) return EG_OK;
  HIPCHK(hipSetDevice(c->device));
  const int depth = egm::depth(n_leaves);
  const MerklePathDev mem{static_cast<const u32*>(d_log), static_cast<const u32*>(d_nodes), static_cast<u32*>(d_paths), egm::HASH_WORDS * (size_t)depth};
  hipLaunchKernelGGL(k_merkle_paths, dim3((unsigned)((m + MERKLE_NT - 1) / MERKLE_NT)), dim3(MERKLE_NT), 0, (hipStream_t)stream, mem,
                     static_cast<const unsigned long long*>(d_index), (uint64_t)m, n_leaves, depth, static_cast<u32*>(d_path_len));
  HIPCHK(hipGetLastError());
  return EG_OK;
}
int eg_merkle_paths(eg_ctx* c, size_t m, const uint64_t* index, uint64_t n_leaves, const uint8_t* log, const uint8_t* nodes, uint8_t* paths,
                    uint32_t* path_len) {
  TRY_(merkle_refuse(egm::refuse_paths(m, n_leaves, index != nullptr, log != nullptr, nodes != nullptr, paths != nullptr, path_len != nullptr)));
  TRY_(check_ctx("merkle", c));
  if (m == 0) return EG_OK;
  HIPCHK(hipSetDevice(c->device));
  HostStage st("merkle"); TRY_(st.open());
  const size_t row = egm::HASH_BYTES * (size_t)egm::depth(n_leaves);
  void *di, *dl = nullptr, *dn = nullptr, *dp = nullptr, *dlen;
  TRY_(st.put(&di, index, m * 8));
  if (n_leaves > 1) {
    TRY_(st.put(&dl, log, (size_t)n_leaves * egm::HASH_BYTES));
    TRY_(st.put(&dn, nodes, eg_merkle_nodes_bytes(n_leaves)));
    TRY_(st.put(&dp, nullptr, m * row));
  }
  TRY_(st.put(&dlen, nullptr, m * 4));
  TRY_(eg_merkle_paths_device(c, m, di, n_leaves, dl, dn, dp, dlen, st.s));
  if (row) TRY_(st.get(paths, dp, m * row));
  TRY_(st.get(path_len, dlen, m * 4));
  TRY_(st.sync());
  return EG_OK;
}

int eg_merkle_check_device(eg_ctx* c, size_t m, const void* d_index, const void* d_leaves, const void* d_paths, size_t path_stride,
                           const void* d_path_len, uint64_t n_leaves, const void* d_root, void* d_verdict, void* d_found, void* stream) {
  TRY_(merkle_refuse(egm::refuse_check(m, n_leaves, d_index != nullptr, d_leaves != nullptr, d_paths != nullptr, path_stride, d_path_len != nullptr,
                                       d_root != nullptr, d_verdict != nullptr, d_found != nullptr)));
  TRY_(check_aligned(MERKLE_ALIGNED, (uintptr_t)d_index, (uintptr_t)d_leaves | (uintptr_t)d_paths | (uintptr_t)d_path_len | (uintptr_t)d_root |
                                                         (uintptr_t)d_verdict | (uintptr_t)d_found));
  TRY_(check_ctx("merkle", c));
  if (!d_found) return EG_OK;                                           // m == 0 and nowhere to write anything to
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  u32* found = static_cast<u32*>(d_found);
  HIPCHK(hipMemsetAsync(found, 0, 3 * sizeof(u32), s));
  if (m == 0) return EG_OK;
  const MerkleCheckDev mem{static_cast<const unsigned long long*>(d_index), static_cast<const u32*>(d_leaves), static_cast<const u32*>(d_paths),
                           path_stride / 4, static_cast<const u32*>(d_path_len), static_cast<const u32*>(d_root)};
  hipLaunchKernelGGL(k_merkle_check, dim3((unsigned)((m + MERKLE_NT - 1) / MERKLE_NT)), dim3(MERKLE_NT), 0, s, mem, (uint64_t)m, n_leaves,
                     static_cast<u32*>(d_verdict), found);
  HIPCHK(hipGetLastError());
  return EG_OK;
}
int eg_merkle_check(eg_ctx* c, size_t m, const uint64_t* index, const uint8_t* leaves, const uint8_t* paths, size_t path_stride,
                    const uint32_t* path_len, uint64_t n_leaves, const uint8_t* root, uint32_t* verdict, uint32_t* found) {
  TRY_(merkle_refuse(egm::refuse_check(m, n_leaves, index != nullptr, leaves != nullptr, paths != nullptr, path_stride, path_len != nullptr,
                                       root != nullptr, verdict != nullptr, found != nullptr)));
  TRY_(check_ctx("merkle", c));
  if (found) found[0] = found[1] = found[2] = 0;
  if (m == 0) return EG_OK;
  HIPCHK(hipSetDevice(c->device));
  HostStage st("merkle"); TRY_(st.open());
  void *di, *dl, *dp = nullptr, *dlen, *dr, *dv, *df;
  TRY_(st.put(&di, index, m * 8));
  TRY_(st.put(&dl, leaves, m * egm::HASH_BYTES));
  if (paths) TRY_(st.put(&dp, paths, m * path_stride));
  TRY_(st.put(&dlen, path_len, m * 4));
  TRY_(st.put(&dr, root, egm::HASH_BYTES));
  TRY_(st.put(&dv, nullptr, m * 4));
  TRY_(st.put(&df, nullptr, 16));
  TRY_(eg_merkle_check_device(c, m, di, dl, dp, path_stride, dlen, n_leaves, dr, dv, df, st.s));
  TRY_(st.get(verdict, dv, m * 4));
  TRY_(st.get(found, df, 3 * sizeof(u32)));
  TRY_(st.sync());
  return EG_OK;
}

// ---- receipt log, the audit entries: past heads, consistency proofs and their check (merkle_audit_kernels.cuh), out of the node store ----
static const AlignedMsgs MERKLE_AUDIT_ALIGNED{"merkle: size and old_size must be 8-byte aligned",
                                              "merkle: log, nodes, heads, proofs, old_root, root, proof_len, verdict and found must be 4-byte aligned"};
uint32_t eg_merkle_consistency_len(uint64_t old_size, uint64_t n_leaves) { return egm::consistency_len(old_size, n_leaves); }

int eg_merkle_heads_device(eg_ctx* c, size_t m, const void* d_size, uint64_t n_leaves, const void* d_log, const void* d_nodes, void* d_heads,
                           void* d_found, void* stream) {
  TRY_(merkle_refuse(egm::refuse_heads(m, n_leaves, d_size != nullptr, d_log != nullptr, d_nodes != nullptr, d_heads != nullptr, d_found != nullptr)));
  TRY_(check_aligned(MERKLE_AUDIT_ALIGNED, (uintptr_t)d_size, (uintptr_t)d_log | (uintptr_t)d_nodes | (uintptr_t)d_heads | (uintptr_t)d_found));
  TRY_(check_ctx("merkle", c));
  if (!d_found) return EG_OK;                                           // m == 0 and nowhere to write anything to
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  u32* found = static_cast<u32*>(d_found);
  HIPCHK(hipMemsetAsync(found, 0, sizeof(u32), s));
  if (m == 0) return EG_OK;
  const MerkleHeadDev mem{static_cast<const unsigned long long*>(d_size), static_cast<const u32*>(d_log), static_cast<const u32*>(d_nodes),
                          static_cast<u32*>(d_heads)};
  hipLaunchKernelGGL(k_merkle_heads, dim3((unsigned)((m + MERKLE_NT - 1) / MERKLE_NT)), dim3(MERKLE_NT), 0, s, mem, (uint64_t)m, n_leaves, found);
  HIPCHK(hipGetLastError());
  return EG_OK;
}
int eg_merkle_heads(eg_ctx* c, size_t m, const uint64_t* size, uint64_t n_leaves, const uint8_t* log, const uint8_t* nodes, uint8_t* heads,
                    uint32_t* found) {
  TRY_(merkle_refuse(egm::refuse_heads(m, n_leaves, size != nullptr, log != nullptr, nodes != nullptr, heads != nullptr, found != nullptr)));
  TRY_(check_ctx("merkle", c));
  if (found) found[0] = 0;
  if (m == 0) return EG_OK;
  HIPCHK(hipSetDevice(c->device));
  HostStage st("merkle"); TRY_(st.open());
  void *ds, *dl = nullptr, *dn = nullptr, *dh, *df;
  TRY_(st.put(&ds, size, m * 8));
  if (n_leaves > 0) TRY_(st.put(&dl, log, (size_t)n_leaves * egm::HASH_BYTES));
  if (n_leaves > 1) TRY_(st.put(&dn, nodes, eg_merkle_nodes_bytes(n_leaves)));
  TRY_(st.put(&dh, nullptr, m * egm::HASH_BYTES));
  TRY_(st.put(&df, nullptr, 16));
  TRY_(eg_merkle_heads_device(c, m, ds, n_leaves, dl, dn, dh, df, st.s));
  TRY_(st.get(heads, dh, m * egm::HASH_BYTES));
  TRY_(st.get(found, df, sizeof(u32)));
  TRY_(st.sync());
  return EG_OK;
}

int eg_merkle_consistency_device(eg_ctx* c, size_t m, const void* d_old_size, uint64_t n_leaves, const void* d_log, const void* d_nodes,
                                 void* d_proofs, void* d_proof_len, void* stream) {
  TRY_(merkle_refuse(egm::refuse_consistency(m, n_leaves, d_old_size != nullptr, d_log != nullptr, d_nodes != nullptr, d_proofs != nullptr,
                                             d_proof_len != nullptr)));
  TRY_(check_aligned(MERKLE_AUDIT_ALIGNED, (uintptr_t)d_old_size, (uintptr_t)d_log | (uintptr_t)d_nodes | (uintptr_t)d_proofs | (uintptr_t)d_proof_len));
  TRY_(check_ctx("merkle", c));
  if (m == 0) return EG_OK;
  HIPCHK(hipSetDevice(c->device));
  const int row = (int)egm::consistency_row(n_leaves);
  const MerkleConsDev mem{static_cast<const u32*>(d_log), static_cast<const u32*>(d_nodes), static_cast<u32*>(d_proofs), egm::HASH_WORDS * (size_t)row};
  hipLaunchKernelGGL(k_merkle_consistency, dim3((unsigned)((m + MERKLE_NT - 1) / MERKLE_NT)), dim3(MERKLE_NT), 0, (hipStream_t)stream, mem,
                     static_cast<const unsigned long long*>(d_old_size), (uint64_t)m, n_leaves, row, static_cast<u32*>(d_proof_len));
  HIPCHK(hipGetLastError());
  return EG_OK;
}
int eg_merkle_consistency(eg_ctx* c, size_t m, const uint64_t* old_size, uint64_t n_leaves, const uint8_t* log, const uint8_t* nodes, uint8_t* proofs,
                          uint32_t* proof_len) {
  TRY_(merkle_refuse(egm::refuse_consistency(m, n_leaves, old_size != nullptr, log != nullptr, nodes != nullptr, proofs != nullptr, proof_len != nullptr)));
  TRY_(check_ctx("merkle", c));
  if (m == 0) return EG_OK;
  HIPCHK(hipSetDevice(c->device));
  HostStage st("merkle"); TRY_(st.open());
  const size_t row = egm::HASH_BYTES * egm::consistency_row(n_leaves);
  void *ds, *dl = nullptr, *dn = nullptr, *dp, *dlen;
  TRY_(st.put(&ds, old_size, m * 8));
  if (n_leaves > 0) TRY_(st.put(&dl, log, (size_t)n_leaves * egm::HASH_BYTES));
  if (n_leaves > 1) TRY_(st.put(&dn, nodes, eg_merkle_nodes_bytes(n_leaves)));
  TRY_(st.put(&dp, nullptr, m * row));
  TRY_(st.put(&dlen, nullptr, m * 4));
  TRY_(eg_merkle_consistency_device(c, m, ds, n_leaves, dl, dn, dp, dlen, st.s));
  TRY_(st.get(proofs, dp, m * row));
  TRY_(st.get(proof_len, dlen, m * 4));
  TRY_(st.sync());
  return EG_OK;
}

int eg_merkle_consistency_check_device(eg_ctx* c, size_t m, const void* d_old_size, const void* d_old_root, const void* d_proofs, size_t proof_stride,
                                       const void* d_proof_len, uint64_t n_leaves, const void* d_root, void* d_verdict, void* d_found, void* stream) {
  TRY_(merkle_refuse(egm::refuse_consistency_check(m, n_leaves, d_old_size != nullptr, d_old_root != nullptr, d_proofs != nullptr, proof_stride,
                                                   d_proof_len != nullptr, d_root != nullptr, d_verdict != nullptr, d_found != nullptr)));
  TRY_(check_aligned(MERKLE_AUDIT_ALIGNED, (uintptr_t)d_old_size, (uintptr_t)d_old_root | (uintptr_t)d_proofs | (uintptr_t)d_proof_len | (uintptr_t)d_root |
                                                                  (uintptr_t)d_verdict | (uintptr_t)d_found));
  TRY_(check_ctx("merkle", c));
  if (!d_found) return EG_OK;                                           // m == 0 and nowhere to write anything to
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  u32* found = static_cast<u32*>(d_found);
  HIPCHK(hipMemsetAsync(found, 0, 4 * sizeof(u32), s));
  if (m == 0) return EG_OK;
  const MerkleConsCheckDev mem{static_cast<const unsigned long long*>(d_old_size), static_cast<const u32*>(d_old_root),
                               static_cast<const u32*>(d_proofs), proof_stride / 4, static_cast<const u32*>(d_proof_len),
                               static_cast<const u32*>(d_root)};
  hipLaunchKernelGGL(k_merkle_cons_check, dim3((unsigned)((m + MERKLE_NT - 1) / MERKLE_NT)), dim3(MERKLE_NT), 0, s, mem, (uint64_t)m, n_leaves,
                     static_cast<u32*>(d_verdict), found);
  HIPCHK(hipGetLastError());
  return EG_OK;
}
int eg_merkle_consistency_check(eg_ctx* c, size_t m, const uint64_t* old_size, const uint8_t* old_root, const uint8_t* proofs, size_t proof_stride,
                                const uint32_t* proof_len, uint64_t n_leaves, const uint8_t* root, uint32_t* verdict, uint32_t* found) {
  TRY_(merkle_refuse(egm::refuse_consistency_check(m, n_leaves, old_size != nullptr, old_root != nullptr, proofs != nullptr, proof_stride,
                                                   proof_len != nullptr, root != nullptr, verdict != nullptr, found != nullptr)));
  TRY_(check_ctx("merkle", c));
  if (found) found[0] = found[1] = found[2] = found[3] = 0;
  if (m == 0) return EG_OK;
  HIPCHK(hipSetDevice(c->device));
  HostStage st("merkle"); TRY_(st.open());
  void *ds, *dor, *dp = nullptr, *dlen, *dr, *dv, *df;
  TRY_(st.put(&ds, old_size, m * 8));
  TRY_(st.put(&dor, old_root, m * egm::HASH_BYTES));
  if (proofs) TRY_(st.put(&dp, proofs, m * proof_stride));
  TRY_(st.put(&dlen, proof_len, m * 4));
  TRY_(st.put(&dr, root, egm::HASH_BYTES));
  TRY_(st.put(&dv, nullptr, m * 4));
  TRY_(st.put(&df, nullptr, 16));
  TRY_(eg_merkle_consistency_check_device(c, m, ds, dor, dp, proof_stride, dlen, n_leaves, dr, dv, df, st.s));
  TRY_(st.get(verdict, dv, m * 4));
  TRY_(st.get(found, df, 4 * sizeof(u32)));
  TRY_(st.sync());
  return EG_OK;
}

// ---- receipt log, the grow entry: the node store of N leaves out of that of its first m (merkle_grow_kernels.cuh; the plan:
// merkle_grow_host.hpp).  One copy launch for the tiles that lie wholly inside the old tree, then the tree's launches from tile0 on ----
static const AlignedMsgs MERKLE_GROW_ALIGNED{"", "merkle: nodes_old, log, nodes and root must be 4-byte aligned"};
int eg_merkle_grow_device(eg_ctx* c, uint64_t old_size, const void* d_nodes_old, uint64_t n_leaves, const void* d_log, void* d_nodes, void* d_root,
                          void* stream) {
  TRY_(merkle_refuse(egm::refuse_grow(old_size, n_leaves, d_nodes_old, d_log != nullptr, d_nodes, d_root != nullptr)));
  TRY_(check_aligned(MERKLE_GROW_ALIGNED, 0, (uintptr_t)d_nodes_old | (uintptr_t)d_log | (uintptr_t)d_nodes | (uintptr_t)d_root));
  TRY_(check_ctx("merkle", c));
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  u32* store = static_cast<u32*>(d_nodes);
  const egm::GrowPlan P = egm::grow_plan(old_size, n_leaves);
  if (P.table.total) {
    const bool wide = (((uintptr_t)d_nodes_old | (uintptr_t)d_nodes) & 15u) == 0;
    const uint64_t units = P.table.total * (wide ? 2u : 8u);
    const unsigned blocks = (unsigned)std::min<uint64_t>((units + MERKLE_NT - 1) / MERKLE_NT, MERKLE_GROW_COPY_BLOCKS);
    hipLaunchKernelGGL(k_merkle_grow_copy, dim3(blocks), dim3(MERKLE_NT), 0, s, MerkleGrowCopyDev{static_cast<const u32*>(d_nodes_old), store},
                       P.table, units, wide ? 1 : 0);
  }
  const u32* cur = n_leaves ? static_cast<const u32*>(d_log) : nullptr;
  for (int k = 0; k < P.n_launches; ++k) {
    const egm::GrowLaunch& g = P.launch[k];
    MerkleTileArgs a;
    a.in = cur; a.n_in = g.n_in; a.store = store; a.top = nullptr; a.steps = g.steps;
    for (int j = 0; j < egm::T_LOG; ++j) a.off[j] = g.off[j];
    if (g.tile0 < g.tiles)
      hipLaunchKernelGGL(k_merkle_grow_tile<egm::T_LOG>, dim3((unsigned)(g.tiles - g.tile0)), dim3(1 << (egm::T_LOG - 2)), 0, s, (u32)g.tile0, a);
    cur = store + g.off[g.steps - 1] * egm::HASH_WORDS;
  }
  hipLaunchKernelGGL(k_merkle_root, dim3(1), dim3(64), 0, s, cur, static_cast<u32*>(d_root));
  HIPCHK(hipGetLastError());
  return EG_OK;
}
int eg_merkle_grow(eg_ctx* c, uint64_t old_size, const uint8_t* nodes_old, uint64_t n_leaves, const uint8_t* log, uint8_t* nodes, uint8_t* root) {
  TRY_(merkle_refuse(egm::refuse_grow(old_size, n_leaves, nodes_old, log != nullptr, nodes, root != nullptr)));
  TRY_(check_ctx("merkle", c));
  HIPCHK(hipSetDevice(c->device));
  HostStage st("merkle"); TRY_(st.open());
  const size_t old_bytes = eg_merkle_nodes_bytes(old_size), store_bytes = eg_merkle_nodes_bytes(n_leaves);
  const uint64_t first = (old_size >> egm::T_LOG) << egm::T_LOG;      // the leaves below are never read: they are not sent either
  void *dl = nullptr, *dno = nullptr, *dn = nullptr, *dr;
  if (n_leaves) {
    TRY_(st.put(&dl, nullptr, (size_t)n_leaves * egm::HASH_BYTES));
    TRY_(h2d(static_cast<char*>(dl) + first * egm::HASH_BYTES, log + first * egm::HASH_BYTES, (size_t)(n_leaves - first) * egm::HASH_BYTES, st.s));
  }
  if (old_bytes) TRY_(st.put(&dno, nodes_old, old_bytes));
  if (store_bytes) TRY_(st.put(&dn, nullptr, store_bytes));
  TRY_(st.put(&dr, nullptr, egm::HASH_BYTES));
  TRY_(eg_merkle_grow_device(c, old_size, dno, n_leaves, dl, dn, dr, st.s));
  TRY_(st.get(root, dr, egm::HASH_BYTES));
  if (store_bytes) TRY_(st.get(nodes, dn, store_bytes));
  TRY_(st.sync());
  return EG_OK;
}

// ---- re-encryption shuffles: the verifier of a mixer's proof (shuffle_kernels.cuh; the rule: include/eg_hip.h) ---------------------------
// Stateless like the receipt log: everything lives in the caller's scratch.  The products go through eg_vartime_multi_mul_batch_device and
// the two roots through eg_merkle_tree_device, as they are; everything is asynchronous on the caller's stream.
static int shuffle_refuse(const char* why) { return why ? fail(EG_ERR_BAD_ARG, std::string("shuffle: ") + why) : EG_OK; }
static egsh::Layout shuffle_layout(const eg_ctx* c, uint64_t n) {
  return egsh::layout(n, (unsigned)c->cus, egm::tree_layout(n).total, msm_scratch_for(c, egsh::BIG_PRODUCTS, 2 * (size_t)n),
                      msm_scratch_for(c, egsh::SMALL_PRODUCTS, egsh::SMALL_TERMS));
}
size_t eg_shuffle_key_bytes(uint64_t cap) { return egsh::key_bytes(cap); }
size_t eg_shuffle_proof_bytes(uint64_t n) { return egsh::proof_bytes(n); }
size_t eg_shuffle_verify_scratch_bytes(const eg_ctx* c, uint64_t n) { return c && n <= egsh::ROWS_MAX ? shuffle_layout(c, n).total : 0; }
int eg_shuffle_key_derive_device(eg_ctx* c, const uint8_t* seed, size_t seed_len, uint64_t cap, void* d_key, void* d_exhausted, void* stream) {
  TRY_(shuffle_refuse(egsh::refuse_key(cap, seed != nullptr, seed_len, d_key != nullptr)));
  if (!d_exhausted) return shuffle_refuse("null exhausted word");
  if (((uintptr_t)d_key | (uintptr_t)d_exhausted) & 3u) return shuffle_refuse("key and the exhausted word must be 4-byte aligned");
  TRY_(check_ctx("shuffle", c));
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  ShufKeyArgs a;
  memset(&a, 0, sizeof a);
  if (seed_len) memcpy(a.seed, seed, seed_len);
  a.seed_len = (u32)seed_len; a.cap = cap; a.tries = egsh::KEY_TRIES;
  HIPCHK(hipMemsetAsync(d_exhausted, 0, sizeof(u32), s));
  hipLaunchKernelGGL(k_shuffle_key, dim3(blocks_of((size_t)cap + 1)), dim3(NT), 0, s, a, static_cast<u32*>(d_key), static_cast<u32*>(d_exhausted));
  HIPCHK(hipGetLastError());
  return EG_OK;
}
int eg_shuffle_key_derive(eg_ctx* c, const uint8_t* seed, size_t seed_len, uint64_t cap, uint8_t* key) {
  TRY_(shuffle_refuse(egsh::refuse_key(cap, seed != nullptr, seed_len, key != nullptr)));
  TRY_(check_ctx("shuffle", c));
  HIPCHK(hipSetDevice(c->device));
  HostStage st("shuffle"); TRY_(st.open());
  void *dk, *de;
  TRY_(st.put(&dk, nullptr, egsh::key_bytes(cap)));
  TRY_(st.put(&de, nullptr, sizeof(u32)));
  TRY_(eg_shuffle_key_derive_device(c, seed, seed_len, cap, dk, de, st.s));
  u32 exhausted = 0;
  TRY_(st.get(key, dk, egsh::key_bytes(cap)));
  TRY_(st.get(&exhausted, de, sizeof exhausted));
  TRY_(st.sync());
  if (exhausted) return shuffle_refuse("a generator found no element within EG_SHUFFLE_KEY_TRIES candidates (its bytes are zero); take another seed");
  return EG_OK;
}
int eg_shuffle_verify_device(eg_ctx* c, uint64_t n, const void* d_in, const void* d_out, const uint8_t* K, const uint8_t* prefix, size_t prefix_len,
                             const void* d_key, uint64_t key_cap, const void* d_proof, void* d_verdict, void* d_rows, void* d_found, void* d_scratch,
                             size_t scratch_bytes, void* stream) {
  TRY_(shuffle_refuse(egsh::refuse_verify(n, key_cap, d_in != nullptr, d_out != nullptr, K != nullptr, prefix != nullptr, prefix_len, d_key != nullptr,
                                          d_proof != nullptr, d_verdict != nullptr, d_found != nullptr)));
  if (((uintptr_t)d_in | (uintptr_t)d_out | (uintptr_t)d_key | (uintptr_t)d_proof | (uintptr_t)d_verdict | (uintptr_t)d_rows | (uintptr_t)d_found) & 3u)
    return shuffle_refuse("in, out, key, proof, verdict, rows and found must be 4-byte aligned");
  if ((uintptr_t)d_scratch & 15u) return shuffle_refuse("scratch must be 16-byte aligned");
  TRY_(check_ctx("shuffle", c));
  const egsh::Layout L = shuffle_layout(c, n);
  if (n && (!d_scratch || scratch_bytes < L.total)) return shuffle_refuse("scratch is null or too small (eg_shuffle_verify_scratch_bytes says how much)");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_shuffle_begin, dim3(1), dim3(64), 0, s, static_cast<u32*>(d_found), static_cast<u32*>(d_verdict));
  if (n == 0) { HIPCHK(hipGetLastError()); return EG_OK; }
  char* base = static_cast<char*>(d_scratch);
  auto words = [&](size_t off) { return reinterpret_cast<u32*>(base + off); };
  ShufDev D;
  D.n = n; D.in = static_cast<const u32*>(d_in); D.out = static_cast<const u32*>(d_out); D.key = static_cast<const u32*>(d_key);
  D.proof = static_cast<const u32*>(d_proof);
  D.prefix = reinterpret_cast<const unsigned char*>(base + L.prefix); D.prefix_len = (u32)prefix_len;
  D.state = words(L.state); D.leaves = words(L.leaves); D.rowbad = reinterpret_cast<unsigned char*>(base + L.rowbad); D.upart = words(L.upart);
  D.big_scalars = words(L.big_scalars); D.big_points = words(L.big_points); D.big_r = words(L.big_r);
  D.small_scalars = words(L.small_scalars); D.small_points = words(L.small_points); D.small_r = words(L.small_r);
  D.rows = static_cast<u32*>(d_rows); D.found = static_cast<u32*>(d_found);
  if (prefix_len) HIPCHK(hipMemcpyAsync(base + L.prefix, prefix, prefix_len, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(D.state + SHUF_ST_K, K, 32, hipMemcpyHostToDevice, s));
  const size_t tree_bytes = egm::tree_layout(n).total;
  const unsigned rb = egsh::row_blocks(n);
  hipLaunchKernelGGL(k_shuffle_leaf1, dim3(rb), dim3(NT), 0, s, D);
  TRY_(eg_merkle_tree_device(c, n, D.leaves, D.state + SHUF_ST_ROOT1, nullptr, base + L.tree, tree_bytes, s));
  hipLaunchKernelGGL(k_shuffle_seed, dim3(1), dim3(64), 0, s, D);
  hipLaunchKernelGGL(k_shuffle_leaf2, dim3(rb), dim3(NT), 0, s, D);
  TRY_(eg_merkle_tree_device(c, n, D.leaves, D.state + SHUF_ST_ROOT2, nullptr, base + L.tree, tree_bytes, s));
  hipLaunchKernelGGL(k_shuffle_x, dim3(1), dim3(64), 0, s, D);
  hipLaunchKernelGGL(k_shuffle_scalars, dim3(rb), dim3(NT), 0, s, D);
  hipLaunchKernelGGL(k_shuffle_fold, dim3(1), dim3(NT), 0, s, D, (u32)rb);
  hipLaunchKernelGGL(k_shuffle_chain, dim3(L.chain_grid), dim3(NT), 0, s, D, (const uint4*)c->tabG, reinterpret_cast<uint4*>(base + L.tables));
  HIPCHK(hipGetLastError());
  const size_t msm_big = msm_scratch_for(c, egsh::BIG_PRODUCTS, 2 * (size_t)n), msm_small = msm_scratch_for(c, egsh::SMALL_PRODUCTS, egsh::SMALL_TERMS);
  TRY_(eg_vartime_multi_mul_batch_device(c, egsh::BIG_PRODUCTS, 2 * (size_t)n, D.big_scalars, D.big_points, D.big_r, msm_big ? base + L.msm : nullptr,
                                         base + L.big_out, base + L.big_ok, s));
  TRY_(eg_vartime_multi_mul_batch_device(c, egsh::SMALL_PRODUCTS, egsh::SMALL_TERMS, D.small_scalars, D.small_points, D.small_r,
                                         msm_small ? base + L.msm : nullptr, base + L.small_out, base + L.small_ok, s));
  hipLaunchKernelGGL(k_shuffle_close, dim3(1), dim3(64), 0, s, D, (const u32*)words(L.big_out), (const unsigned char*)(base + L.big_ok),
                     (const u32*)words(L.small_out), (const unsigned char*)(base + L.small_ok), static_cast<u32*>(d_verdict));
  HIPCHK(hipGetLastError());
  return EG_OK;
}
int eg_shuffle_verify(eg_ctx* c, uint64_t n, const uint8_t* in, const uint8_t* out, const uint8_t* K, const uint8_t* prefix, size_t prefix_len,
                      const uint8_t* key, uint64_t key_cap, const uint8_t* proof, uint32_t* verdict, uint32_t* rows, uint32_t* found) {
  TRY_(shuffle_refuse(egsh::refuse_verify(n, key_cap, in != nullptr, out != nullptr, K != nullptr, prefix != nullptr, prefix_len, key != nullptr,
                                          proof != nullptr, verdict != nullptr, found != nullptr)));
  TRY_(check_ctx("shuffle", c));
  HIPCHK(hipSetDevice(c->device));
  HostStage st("shuffle"); TRY_(st.open());
  const size_t need = eg_shuffle_verify_scratch_bytes(c, n);
  void *di = nullptr, *dout = nullptr, *dk = nullptr, *dp = nullptr, *dv, *dr = nullptr, *df, *scratch = nullptr;
  if (n) {
    TRY_(st.put(&di, in, (size_t)n * 64)); TRY_(st.put(&dout, out, (size_t)n * 64));
    TRY_(st.put(&dk, key, ((size_t)n + 1) * 32));                      // the generators behind H_N are never read
    TRY_(st.put(&dp, proof, egsh::proof_bytes(n)));
    if (rows) TRY_(st.put(&dr, nullptr, (size_t)n * 4));
    TRY_(st.put(&scratch, nullptr, need));
  }
  TRY_(st.put(&dv, nullptr, 4)); TRY_(st.put(&df, nullptr, 16));
  TRY_(eg_shuffle_verify_device(c, n, di, dout, K, prefix, prefix_len, dk, key_cap, dp, dv, dr, df, scratch, need, st.s));
  TRY_(st.get(verdict, dv, 4)); TRY_(st.get(found, df, 16));
  if (n && rows) TRY_(st.get(rows, dr, (size_t)n * 4));
  TRY_(st.sync());
  return EG_OK;
}

}  // extern "C"
