// C-ABI of libpcabo.so (declared in include/pcabo.h): context management, host<->device staging and
// the launch sequences of the wPCA / GP-conditioning / acquisition phases.
#include "../../include/pcabo.h"
#include "pcabo_internal.h"
#include "lbfgsb.h"
#include "host_side.h"
#include "model_state.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <optional>
#include <vector>
#include <dirent.h>
#include <fcntl.h>
#include <signal.h>
#include <stdint.h>
#include <cerrno>
#include <unistd.h>
#include <emmintrin.h>

#define PCABO_ABI_VERSION 2
#define PROF_GROUPS 6
#define PROF_POOL 4096

struct ProfPair { hipEvent_t a, b; int group; double bytes, flops; };

struct pcabo_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t evBounds = nullptr;         // recorded after k_zstats: the search box is on the host before the Cholesky ends
  hipEvent_t evPca = nullptr;            // recorded after the wPCA results left for the host (conditioning may follow it)
  // PCABO_OPT_HIDDEN_TAIL, single contexts: the raw samples' copy and their kernel vectors (k_score_ks_only) run on a second stream
  // beside the factorisation.  evZn: recorded behind k_znorm on the main stream, the second stream waits for it; evKS: recorded
  // behind the kernel vectors, the main stream waits for it in front of the launches that need them.
  hipStream_t stream2 = nullptr;
  hipEvent_t evZn = nullptr, evKS = nullptr;
  bool opt_hidden_tail = true;
  int max_n = 0, max_d = 0, max_q = 0;
  CtxLayout lay{};                       // shape (lay.s: the padded capacities) and layout of the two regions (ctx_layout.h)
  int ld = 0;
  int ptr_mode = PCABO_PTR_HOST;
  ModelState st;                         // where the model stands (model_state.h): read here, changed by its transitions only
  // device buffers
  double *dX = nullptr, *dNoise = nullptr, *dF = nullptr, *dWeights = nullptr, *dWc = nullptr;
  long long* dRanks = nullptr;
  double *dDataMean = nullptr, *dPcaMean = nullptr, *dC = nullptr, *dLam = nullptr;
  double* dGbuf[2] = {nullptr, nullptr};   // eigenvector ping-pong (st.gcur): the previous result warm-starts the next Jacobi
  double *dComps = nullptr, *dEvr = nullptr, *dZ = nullptr;
  double* dPcaOut = nullptr;             // [data_mean | pca_mean | evr | comps]: one allocation, one copy to the host
  double *dIn = nullptr, *hIn = nullptr; // host-pointer mode: X, noise, ranks (or f) and y travel packed in ONE copy
  int *dK = nullptr, *dSweeps = nullptr, *dInfo = nullptr;
  double *dY = nullptr, *dYs = nullptr, *dYstats = nullptr, *dBounds4 = nullptr, *dZnMean = nullptr, *dUserNB = nullptr;
  double *dZnT = nullptr, *dAT = nullptr, *dNrm = nullptr, *dGram = nullptr, *dL = nullptr, *dR = nullptr;
  double *dTmp = nullptr, *dAlpha = nullptr, *dDiag = nullptr;   // dDiag: 64x64 hand-over tile of the Cholesky panels
  double *dXq = nullptr, *dPartial = nullptr, *dVal = nullptr, *dGrad = nullptr, *dZq = nullptr, *dXout = nullptr;
  unsigned int* dCounters = nullptr;     // per-query tickets of the in-launch combine (st.cnt_S, st.cnt_dirty)
  double* dKS = nullptr;                 // q x ld kernel vectors of the GEMM scoring path
  double* dBestF = nullptr;              // best_f of this run for the batched acquisition launches (set by the batch)
  double* dMll = nullptr;                // GP fit: 1 + M partial sums per lower 64 x 64 tile of K^-1, then the 5 + M results
                                         // (k_mll_finish); M = 1, ARD: M = KP
  double* dArdLs = nullptr;              // ARD fit: the k lengthscales k_zstats folds into the Normalize ranges
  double* dHyp = nullptr;                // lock-step fit of a batch: this run's {1 / lengthscale, noise, mean constant} (PCABO_HYP_*)
  char* dPostV = nullptr;                // pcabo_gp_posterior with a covariance: V (NPcap x max_q), then cov (max_q^2); allocated
                                         // by the first such call, kept until destroy
  char* dSample = nullptr;               // pcabo_gp_posterior_sample: the sample block (SampleBlock), allocated by the first such call
  char *dRegion = nullptr, *hRegion = nullptr;   // the two allocations everything above / below is carved from
  bool in_batch = false; int batch_index = 0;
  // pinned host
  HostMirror* hm = nullptr;
  double *hXq = nullptr, *hVal = nullptr, *hGrad = nullptr, *hSmall = nullptr, *hBestF = nullptr;
  double* hMll = nullptr;                // GP fit: the 6 results of one evaluation (ARD: 5 + KP)
  double* hArdLs = nullptr;              // ARD fit: the lengthscales on their way to dArdLs
  double* hHyp = nullptr;                // lock-step fit of a batch: the host copy of dHyp
  MailPair* dMail = nullptr;             // mailbox of the resident acquisition kernel, in device memory
  bool mail_bar = false;                 // the host can write dMail itself through the PCIe BAR (the resident mode needs it)
  MailPair* dPairs = nullptr;            // its partial records as (value, tag) pairs: 32 queries x 32 slabs
  bool opt_resident = true;             // PCABO_OPT_RESIDENT: may pcabo_optimize_acqf use the resident acquisition kernel
  bool opt_group_acq = false;           // PCABO_OPT_GROUP_ACQ: gradient evaluations through k_acq_group (throughput variant)
  bool bestf_f32 = true;                // PCABO_OPT_BESTF_F32: best_f rounded like torch.as_tensor(python float)
  int srv_penalty = 0;                   // > 0: the next calls use plain launches (the GPU looked shared, see ResidentSession)
  unsigned long long seq = 0;
  OptCrew crew;                          // the helper threads of pcabo_optimize_acqf (host_side.h)
  double first_advance_s = 0.0;          // the last optimise call's first advance_all, host seconds (pcabo_debug_first_advance_seconds)
  bool registered = false;
  bool alone = true; int alone_age = 0;   // cached answer of presence_alone(), refreshed every few calls
  char err[512] = {0};
  // profiling
  bool prof = false;
  std::vector<ProfPair> pairs;
  size_t pairs_used = 0;
  double prof_ms[PROF_GROUPS] = {0};
  double prof_pair_ms = 0.0;             // reading of two events recorded back to back (calibrated when profiling is enabled)
  double prof_empty_ms = 0.0;            // reading of an event pair around an empty kernel
  int64_t prof_launches[PROF_GROUPS] = {0};
  double prof_bytes[PROF_GROUPS] = {0}, prof_flops[PROF_GROUPS] = {0};
};

// ---- who else drives this GPU?  ---------------------------------------------------------------------------------
// The resident acquisition kernel holds most of the chip for a whole optimize call.  That is the fastest way to run ONE
// process per GPU (the contract of this package), but when several processes share a device their resident kernels can
// only run one after the other, whole calls at a time (measured: 4 processes 140 instead of 336 it/s in aggregate).
// Every process therefore leaves a marker /dev/shm/pcabo.<device>.<pid> while it has a context on a device, and the
// resident mode is used only by a process that finds itself alone there (markers of dead processes are removed).
static std::mutex g_presence_mu;
static int g_presence_refs[64] = {0};
static void presence_path(char* buf, size_t n, int device, long pid) { snprintf(buf, n, "/dev/shm/pcabo.%d.%ld", device, pid); }
static void presence_register(int device) {
  if (device < 0 || device >= 64) return;
  std::lock_guard<std::mutex> lk(g_presence_mu);
  if (g_presence_refs[device]++ == 0) {
    char path[128]; presence_path(path, sizeof(path), device, (long)getpid());
    int fd = open(path, O_CREAT | O_WRONLY, 0644);
    if (fd >= 0) close(fd);
  }
}
static void presence_unregister(int device) {
  if (device < 0 || device >= 64) return;
  std::lock_guard<std::mutex> lk(g_presence_mu);
  if (g_presence_refs[device] > 0 && --g_presence_refs[device] == 0) {
    char path[128]; presence_path(path, sizeof(path), device, (long)getpid());
    unlink(path);
  }
}
// contexts of THIS process on the device (stand-alone ones and the members of batches alike)
static int presence_local_contexts(int device) {
  if (device < 0 || device >= 64) return 1;
  std::lock_guard<std::mutex> lk(g_presence_mu);
  return g_presence_refs[device];
}
static bool presence_alone(int device) {
  DIR* d = opendir("/dev/shm");
  if (!d) return true;
  char prefix[64]; snprintf(prefix, sizeof(prefix), "pcabo.%d.", device);
  const size_t pl = strlen(prefix);
  bool alone = true;
  while (struct dirent* e = readdir(d)) {
    if (strncmp(e->d_name, prefix, pl) != 0) continue;
    const long pid = atol(e->d_name + pl);
    if (pid <= 0 || pid == (long)getpid()) continue;
    if (kill((pid_t)pid, 0) == 0 || errno == EPERM) { alone = false; break; }
    char path[300]; snprintf(path, sizeof(path), "/dev/shm/%s", e->d_name);
    unlink(path);                                   // left behind by a process that is gone
  }
  closedir(d);
  return alone;
}

static int set_err(pcabo_ctx* c, int code, const char* fmt, const char* a = "", int v = 0) {
  if (c) snprintf(c->err, sizeof(c->err), fmt, a, v);
  if (c && (code == PCABO_ERR_TIMEOUT || code == PCABO_ERR_HIP)) c->st.launch_may_have_died();
  return code;
}
#define HIPCHK(call)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) return set_err(ctx, PCABO_ERR_HIP, "HIP error: %s (line %d)", hipGetErrorString(e_), __LINE__); \
  } while (0)

// ---- waiting for the device -----------------------------------------------------------------------------------
// hipStreamSynchronize / hipEventSynchronize put the calling thread to sleep once the wait lasts longer than the
// runtime's short active-wait window; it then comes back late and cold (measured: the first ~0.15 ms of host work after a
// 0.2 ms wait ran several times slower).  The waits of a BO iteration are 0.1-0.4 ms, so they poll instead, and only a
// wait that lasts longer than 2 ms falls back to the blocking call.
static hipError_t wait_stream(hipStream_t s) {
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 1;; ++spins) {
    hipError_t e = hipStreamQuery(s);
    if (e != hipErrorNotReady) return e == hipSuccess ? hipStreamSynchronize(s) : e;
    if ((spins & 63) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    __builtin_ia32_pause();
  }
  return hipStreamSynchronize(s);
}
static hipError_t wait_event(hipEvent_t ev) {
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 1;; ++spins) {
    hipError_t e = hipEventQuery(ev);
    if (e != hipErrorNotReady) return e;
    if ((spins & 63) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    __builtin_ia32_pause();
  }
  return hipEventSynchronize(ev);
}
// Spin until the host mirror's qflag[q0 .. q0 + nq) all carry seq (the launch that writes them has published its results) or the
// deadline passes; given a stream, also stop once that stream has finished while a flag is still missing.
enum FlagWait { FLAGS_SET, FLAGS_LATE, FLAGS_UNPUBLISHED };
static FlagWait wait_flags(const HostMirror* hm, int q0, int nq, unsigned long long seq,
                           std::chrono::steady_clock::time_point deadline, const hipStream_t* s = nullptr) {
  unsigned long spins = 0;
  for (int q = q0; q < q0 + nq; ++q)
    while (__atomic_load_n(&hm->qflag[q], __ATOMIC_ACQUIRE) != seq) {
      if ((++spins & 0xFFFF) != 0) continue;
      if (s && hipStreamQuery(*s) == hipSuccess) {              // the launch is over: the flag must be there
        if (__atomic_load_n(&hm->qflag[q], __ATOMIC_ACQUIRE) == seq) break;
        return FLAGS_UNPUBLISHED;
      }
      if (std::chrono::steady_clock::now() > deadline) return FLAGS_LATE;
    }
  return FLAGS_SET;
}
static std::chrono::steady_clock::time_point deadline_in(int seconds) {
  return std::chrono::steady_clock::now() + std::chrono::seconds(seconds);
}

// ---- the resident kernel's mailbox, written by the host straight into device memory --------------------------------
// With a large PCIe BAR the CPU can address device memory.  The host then stores the round's (value, tag) pairs into the
// DEVICE mailbox itself (16-byte stores, write-combined, one sfence) and the relay work-group that used to fetch them
// from pinned host memory over PCIe has nothing to do: 5.5 -> 4.6 us per round trip in profiles/tools/bar_mailbox_rtt.hip.
// Used when the device reports a large BAR, the process maps the mailbox read-write (/proc/self/maps - no store is tried
// otherwise, no fault is caught) AND a probe store is read back from the device.  Without it there is no resident mode
// (round 1's relay work-group, which fetched the pairs from pinned host memory, is gone): one launch per evaluation.
static inline void put_mail_pair(MailPair* dst, double v, unsigned long long seq) {
  unsigned long long vb; memcpy(&vb, &v, 8);
  const __m128i x = _mm_set_epi64x((long long)(seq ^ mail_mix(vb)), (long long)vb);
  _mm_store_si128(reinterpret_cast<__m128i*>(dst), x);        // value and tag leave in one store
}
// Can the CPU store to [p, p+len)?  Answered from /proc/self/maps: on a large-BAR system the runtime maps device
// allocations into the process read-write; without host access the range is reserved without write permission.  No
// store is attempted unless the mapping says it is allowed, so nothing can fault and no signal handler is touched.
static bool host_mapping_writable(const void* p, size_t len) {
  FILE* f = fopen("/proc/self/maps", "r");
  if (!f) return false;
  const unsigned long long a = (unsigned long long)(uintptr_t)p, b = a + len;
  char line[512];
  bool ok = false;
  while (fgets(line, sizeof(line), f)) {
    unsigned long long lo = 0, hi = 0;
    char perms[8] = {0};
    if (sscanf(line, "%llx-%llx %7s", &lo, &hi, perms) != 3) continue;
    if (a >= lo && b <= hi) { ok = perms[0] == 'r' && perms[1] == 'w'; break; }
  }
  fclose(f);
  return ok;
}
static bool mail_bar_usable(pcabo_ctx* ctx) {
  int large = 0;
  if (hipDeviceGetAttribute(&large, hipDeviceAttributeIsLargeBar, ctx->device) != hipSuccess) { (void)hipGetLastError(); large = 0; }
  if (!large) return false;
  if (!host_mapping_writable(ctx->dMail, PCABO_MAIL_PAIRS * sizeof(MailPair))) return false;
  // the mapping is writable: verify that a store through it is what the device sees (read back with a copy)
  MailPair* probe = ctx->dMail + (PCABO_MAIL_PAIRS - 1);
  put_mail_pair(probe, 42.5, 0x1234ull);
  _mm_sfence();
  MailPair back{0.0, 0};
  if (hipMemcpy(&back, probe, sizeof(back), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return false; }
  unsigned long long vb; const double v = 42.5; memcpy(&vb, &v, 8);
  const bool seen = back.v == 42.5 && back.tag == (0x1234ull ^ mail_mix(vb));
  put_mail_pair(probe, 0.0, 0); _mm_sfence();
  return seen;
}

// ---- profiling helpers ------------------------------------------------------------------------
__global__ void k_nop() {}

static void prof_resolve(pcabo_ctx* c) {
  if (c->pairs_used == 0) return;
  (void)hipStreamSynchronize(c->stream);
  for (size_t i = 0; i < c->pairs_used; ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->pairs[i].a, c->pairs[i].b) == hipSuccess) {
      // two events recorded back to back already read c->prof_pair_ms; the rest is attributed to the launch
      ms = ms > (float)c->prof_pair_ms ? ms - (float)c->prof_pair_ms : 0.f;
      c->prof_ms[c->pairs[i].group] += ms;
      c->prof_launches[c->pairs[i].group] += 1;
      c->prof_bytes[c->pairs[i].group] += c->pairs[i].bytes;
      c->prof_flops[c->pairs[i].group] += c->pairs[i].flops;
    }
  }
  c->pairs_used = 0;
}
struct ProfScope {
  pcabo_ctx* c; ProfPair* p = nullptr;
  // bytes / flops: ALGORITHMIC work of the bracketed launches (formulas in DESIGN.md section 4)
  ProfScope(pcabo_ctx* ctx, int group, double bytes = 0.0, double flops = 0.0) : c(ctx) {
    if (!c->prof) return;
    if (c->pairs_used == c->pairs.size()) prof_resolve(c);
    p = &c->pairs[c->pairs_used++];
    p->group = group; p->bytes = bytes; p->flops = flops;
    (void)hipEventRecord(p->a, c->stream);
  }
  ~ProfScope() { if (p) (void)hipEventRecord(p->b, c->stream); }
};

// ---- algorithmic work models (per launch), see DESIGN.md section 4 ----------------------------
static double acq_bytes(int n, int k, int q, int grad) {
  return 4.0 * n * (n + 1.0) + 8.0 * n * k + 8.0 * n + 8.0 * q * k + 8.0 * q * (grad ? 1 + k : 1);
}
static double acq_flops(int n, int k, int q, int grad) {
  double v = 3.0 * n * k + 20.0 * n + (double)n * n;          // ks, mu, v = R ks (triangular)
  if (grad) v += (double)n * n + 4.0 * n * k;                   // w = R^T v, contraction with dks/dx
  return q * v;
}

template <typename T>
static hipError_t dalloc(T** p, size_t count) { return hipMalloc((void**)p, count * sizeof(T)); }

extern "C" {

int pcabo_abi_version(void) { return PCABO_ABI_VERSION; }

int pcabo_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

}  // extern "C" (helpers with C++ linkage follow)

// ---- memory of a context --------------------------------------------------------------------------------------------
// The context's pointers from its layout (ctx_layout.h: the two regions, every buffer's offset, and who else uses a buffer)
static void ctx_bind(pcabo_ctx* ctx) {
  const CtxLayout& L = ctx->lay;
  const auto D = [&](DevBuf b) { return buf_at<double>(ctx->dRegion, L.dev[b]); };
  const auto I = [&](DevBuf b) { return buf_at<int>(ctx->dRegion, L.dev[b]); };
  const auto H = [&](HostBuf b) { return buf_at<double>(ctx->hRegion, L.host[b]); };
  ctx->dX = D(D_X);             ctx->dNoise = D(D_NOISE);   ctx->dF = D(D_F);           ctx->dWeights = D(D_WEIGHTS);
  ctx->dWc = D(D_WC);           ctx->dRanks = buf_at<long long>(ctx->dRegion, L.dev[D_RANKS]);
  const PcaParts pp = pca_parts(L.s);
  ctx->dPcaOut = D(D_PCAOUT);
  ctx->dDataMean = ctx->dPcaOut + pp.data_mean; ctx->dPcaMean = ctx->dPcaOut + pp.pca_mean; ctx->dEvr = ctx->dPcaOut + pp.evr;
  ctx->dComps = ctx->dPcaOut + pp.comps;
  ctx->dIn = D(D_IN);           ctx->dC = D(D_C);           ctx->dGbuf[0] = D(D_G0);    ctx->dGbuf[1] = D(D_G1);
  ctx->dLam = D(D_LAM);         ctx->dZ = D(D_Z);
  ctx->dK = I(D_K);             ctx->dSweeps = I(D_SWEEPS); ctx->dInfo = I(D_INFO);
  ctx->dY = D(D_Y);             ctx->dYs = D(D_YS);         ctx->dYstats = D(D_YSTATS); ctx->dBounds4 = D(D_BOUNDS4);
  ctx->dZnMean = D(D_ZNMEAN);   ctx->dUserNB = D(D_USERNB); ctx->dZnT = D(D_ZNT);       ctx->dAT = D(D_AT);
  ctx->dNrm = D(D_NRM);         ctx->dGram = D(D_GRAM);     ctx->dL = D(D_L);           ctx->dR = D(D_R);
  ctx->dTmp = D(D_TMP);         ctx->dAlpha = D(D_ALPHA);   ctx->dDiag = D(D_DIAG);
  ctx->dXq = D(D_XQ);           ctx->dPartial = D(D_PARTIAL); ctx->dVal = D(D_VAL);     ctx->dGrad = D(D_GRAD);
  ctx->dZq = D(D_ZQ);           ctx->dXout = D(D_XOUT);     ctx->dBestF = D(D_BESTF);   ctx->dKS = D(D_KS);
  ctx->dCounters = buf_at<unsigned int>(ctx->dRegion, L.dev[D_COUNTERS]);
  ctx->dMll = D(D_MLL);         ctx->dArdLs = D(D_ARDLS);   ctx->dHyp = D(D_HYP);
  ctx->hm = buf_at<HostMirror>(ctx->hRegion, L.host[H_MIRROR]);
  ctx->hXq = H(H_XQ);           ctx->hVal = H(H_VAL);       ctx->hGrad = H(H_GRAD);     ctx->hSmall = H(H_SMALL);
  ctx->hIn = H(H_IN);           ctx->hBestF = H(H_BESTF);   ctx->hMll = H(H_MLL);       ctx->hArdLs = H(H_ARDLS);
  ctx->hHyp = H(H_HYP);
}
// a use of hSmall in one run's block; the bytes of a run's ticket array
static double* small_at(const pcabo_ctx* ctx, Use u) { return ctx->hSmall + u.start; }
static size_t ticket_bytes(const pcabo_ctx* ctx) { return ctx->lay.dev[D_COUNTERS].count * sizeof(unsigned int); }

// Fill in a context over (optionally) somebody else's memory and stream: `dreg` / `hreg` / `stream` non-null = a member
// of a batch (no resident-mode buffers, nothing owned).
static int ctx_setup(pcabo_ctx* ctx, int device, const CtxLayout& lay, char* dreg, char* hreg, hipStream_t stream) {
  ctx->device = device;
  ctx->lay = lay;
  ctx->max_n = lay.s.max_n; ctx->max_d = lay.s.max_d; ctx->max_q = lay.s.max_q;
  ctx->ld = lay.s.NPcap;
  ctx->in_batch = dreg != nullptr;
  HIPCHK(hipSetDevice(device));
  if (stream) ctx->stream = stream;
  else HIPCHK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
  presence_register(ctx->device); ctx->registered = true;
  HIPCHK(hipEventCreateWithFlags(&ctx->evBounds, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&ctx->evPca, hipEventDisableTiming));
  if (!stream) {
    HIPCHK(hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&ctx->evZn, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&ctx->evKS, hipEventDisableTiming));
  }
  if (dreg) {
    ctx->dRegion = dreg; ctx->hRegion = hreg;        // zeroed by the batch
  } else {
    HIPCHK(hipMalloc((void**)&ctx->dRegion, lay.dev_bytes));
    HIPCHK(hipHostMalloc((void**)&ctx->hRegion, lay.host_bytes, hipHostMallocDefault));
    memset(ctx->hRegion, 0, lay.host_bytes);
  }
  ctx_bind(ctx);
  if (!dreg) {
    // zero: the per-query tickets, the padded tail of y_s, and R (its blocks above the diagonal stay zero for good)
    HIPCHK(hipMemsetAsync(ctx->dRegion, 0, lay.dev_bytes, ctx->stream));
    if (hipExtMallocWithFlags((void**)&ctx->dMail, PCABO_MAIL_PAIRS * sizeof(MailPair), hipDeviceMallocFinegrained) != hipSuccess) {
      (void)hipGetLastError();
      HIPCHK(dalloc(&ctx->dMail, PCABO_MAIL_PAIRS));
    }
    HIPCHK(hipMemsetAsync(ctx->dMail, 0, PCABO_MAIL_PAIRS * sizeof(MailPair), ctx->stream));
    const size_t np = (size_t)PCABO_INLAUNCH_MAXQ * 32 * (2 + 2 * PCABO_MAXD);
    HIPCHK(dalloc(&ctx->dPairs, np));
    HIPCHK(hipMemsetAsync(ctx->dPairs, 0, np * sizeof(MailPair), ctx->stream));   // on OUR stream: a memset on the
    // null stream is not ordered with the non-blocking streams the resident kernels run on
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->mail_bar = mail_bar_usable(ctx);
  } else {
    ctx->opt_resident = false;           // the resident kernel wants most of the chip for one run: not inside a batch
  }
  // Sequence numbers double as mailbox tags.  Memory handed out by the allocator may come from a context that was
  // destroyed earlier in this process, so every context numbers from its own base: a stale tag can never match.
  {
    static std::atomic<unsigned long long> ctx_counter{0};
    ctx->seq = ((unsigned long long)(getpid() & 0xffff) << 44) + ((ctx_counter.fetch_add(1) + 1) << 30);
  }
  return PCABO_OK;
}

static void ctx_teardown(pcabo_ctx* ctx) {
  (void)hipSetDevice(ctx->device);        // tear-down: nothing useful to do with an error from here on
  if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  for (auto& p : ctx->pairs) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
  if (!ctx->in_batch) {
    if (ctx->dRegion) (void)hipFree(ctx->dRegion);
    if (ctx->hRegion) (void)hipHostFree(ctx->hRegion);
    if (ctx->dMail) (void)hipFree(ctx->dMail);
    if (ctx->dPairs) (void)hipFree(ctx->dPairs);
  }
  if (ctx->dPostV) (void)hipFree(ctx->dPostV);
  if (ctx->dSample) (void)hipFree(ctx->dSample);
  if (ctx->evBounds) (void)hipEventDestroy(ctx->evBounds);
  if (ctx->evPca) (void)hipEventDestroy(ctx->evPca);
  if (ctx->evZn) (void)hipEventDestroy(ctx->evZn);
  if (ctx->evKS) (void)hipEventDestroy(ctx->evKS);
  if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
  if (ctx->stream && !ctx->in_batch) (void)hipStreamDestroy(ctx->stream);
  ctx->crew.shutdown();
  if (ctx->registered) presence_unregister(ctx->device);
}

// ---- rows D-H: ONE launch sequence for a single context and for the B runs of a batch -----------------------------------
// ctx = the context, or run 0 of a batch with zb = its strides (blockIdx.z = run).  phase(1..4) is called at the four cuts of the
// sequence - before k_zstats, before the Cholesky, before the root inverse, behind alpha - and returns PCABO_OK (0) or an error that
// ends the sequence: a caller puts there what it has at that place in stream order (its profiling marks; behind alpha the launches
// that go in front of the copy of chol_info).  Errors are left in ctx.
struct RowsDH {
  const double *Z, *y, *unb;             // the points, the targets, the user's Normalize bounds (or null) on the device
  int n, k, KP; const int* k_dev;        // k and KP by value, or k_dev: read on the device
  double inv_ls, noise, mean_c; int kernel;   // by value (zero where zb.hyp carries every run's own)
  ZB zb;
  hipEvent_t ev[2];                      // recorded behind k_zstats (null: none): the search box is on its way to the host
  bool reset_tickets;                    // the owner's record asked for it (tickets_need_reset) and has been told (tickets_reset)
  const double* ard_ls = nullptr;        // ARD fit: k lengthscales on the device, folded by k_zstats (inv_ls = 1); a batch: run 0's,
                                         // every run's own where its zb.hyp block has PCABO_HYP_ARD_FOLD set
  hipEvent_t ev_zn = nullptr;            // recorded behind k_znorm (null: none): ZnT and the Normalize bounds are final
};
template <class Phase>
static int enqueue_factor(pcabo_ctx* ctx, hipStream_t s, int n, int NP, ZB zb, Phase&& phase) {
  if (const int rc = phase(2)) return rc;
  // a single context folds the root inverse into the panel launches (PCABO_OPT_HIDDEN_TAIL); a batch keeps the separate launches
  const bool fold = !ctx->in_batch && ctx->opt_hidden_tail && zb.zs == 0 && zb.B == 1 && chol_step_form(NP, zb);
  if (launch_cholesky(s, ctx->dL, NP, ctx->ld, ctx->dInfo, ctx->dDiag, zb, fold ? ctx->dR : nullptr) != 0)
    return set_err(ctx, PCABO_ERR_HIP, "the Cholesky launches could not be set up (device or kernel attribute)%s", "");
  if (const int rc = phase(3)) return rc;
  if (fold) launch_trinv_drain(s, ctx->dL, NP, ctx->ld, ctx->dR);
  else launch_trinv(s, ctx->dL, NP, ctx->ld, ctx->dR, zb);
  launch_alpha(s, ctx->dR, ctx->dYs, n, NP, ctx->ld, ctx->dTmp, ctx->dAlpha, zb);
  if (const int rc = phase(4)) return rc;
  if (zb.zs) HIPCHK(hipMemcpy2DAsync((void*)&ctx->hm->chol_info, zb.hzs, ctx->dInfo, zb.zs, sizeof(int), zb.B, hipMemcpyDeviceToHost, s));
  else HIPCHK(hipMemcpyAsync((void*)&ctx->hm->chol_info, ctx->dInfo, sizeof(int), hipMemcpyDeviceToHost, s));
  return PCABO_OK;
}
template <class Phase>
static int enqueue_rows_dh(pcabo_ctx* ctx, hipStream_t s, const RowsDH& a, Phase&& phase) {
  const int NP = round_up(a.n, PCABO_BS);
  if (a.reset_tickets) {
    if (a.zb.zs) HIPCHK(hipMemset2DAsync(ctx->dCounters, a.zb.zs, 0, ticket_bytes(ctx), a.zb.B, s));
    else HIPCHK(hipMemsetAsync(ctx->dCounters, 0, ticket_bytes(ctx), s));
  }
  if (const int rc = phase(1)) return rc;
  launch_zstats(s, a.Z, a.y, a.n, a.k, a.unb, ctx->dBounds4, ctx->dZnMean, ctx->dYstats, ctx->dYs, ctx->hm, a.k_dev, a.zb, a.mean_c, a.ard_ls);
  for (hipEvent_t e : a.ev) if (e) HIPCHK(hipEventRecord(e, s));
  launch_znorm(s, a.Z, a.n, a.k, NP, a.KP, ctx->ld, ctx->dBounds4, ctx->dZnMean, a.inv_ls, ctx->dZnT, ctx->dAT, ctx->dNrm, a.k_dev, a.zb);
  if (a.ev_zn) HIPCHK(hipEventRecord(a.ev_zn, s));
  launch_gram(s, ctx->dAT, ctx->dNrm, a.n, NP, a.KP, ctx->ld, a.noise, a.kernel, nullptr, a.k_dev, ctx->dL, ctx->dInfo, a.zb);
  return enqueue_factor(ctx, s, a.n, NP, a.zb, phase);
}

// ---- rows A-C: the weighted PCA of one BO iteration, its inputs on the device --------------------------------------------------------
struct WpcaInputs { const double *X, *noise, *y; const long long* ranks; };
// ONE launch sequence for a single context and for the B runs of a batch, like enqueue_rows_dh: ctx = the context, or run 0 of a
// batch with zb = its strides; st = the owner's record (the ping-pong of the eigenvectors); ev = the owner's evPca.  mark(0) is
// called in front of the launches and mark(1) behind them: the caller's profiling marks at those places in stream order.
template <class Mark>
static int enqueue_rows_ac(pcabo_ctx* ctx, hipStream_t s, ModelState& st, const WpcaInputs& in, int n, int d, double var_threshold,
                           int n_components, ZB zb, hipEvent_t ev, Mark&& mark) {
  const int DP = round_up(d, 16);
  mark(0);
  launch_wpca_prep(s, in.X, in.ranks, in.noise, n, d, DP, ctx->dWeights, ctx->dDataMean, ctx->dPcaMean, ctx->dWc, zb);
  launch_cov(s, ctx->dWc, n, DP, ctx->dC, zb);
  const double* v0 = st.warm_start(d) ? ctx->dGbuf[st.gcur] : nullptr;
  st.wpca_enqueued(n, d);                // (flips the ping-pong: this Jacobi writes the other buffer)
  launch_jacobi(s, ctx->dC, d, DP, v0, ctx->dGbuf[st.gcur], ctx->dLam, ctx->dSweeps, n, var_threshold, n_components, ctx->dComps,
                ctx->dEvr, ctx->dK, ctx->hm, zb);
  launch_project(s, in.X, ctx->dDataMean, ctx->dPcaMean, ctx->dComps, ctx->dK, n, d, ctx->dZ, zb);
  mark(1);
  const size_t bytes = pca_copy_count(ctx->lay.s, n < d ? n : d, d) * sizeof(double);
  double* h = small_at(ctx, small_wpca(ctx->lay.s));
  if (zb.zs) HIPCHK(hipMemcpy2DAsync(h, zb.hzs, ctx->dPcaOut, zb.zs, bytes, zb.B, hipMemcpyDeviceToHost, s));
  else HIPCHK(hipMemcpyAsync(h, ctx->dPcaOut, bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipEventRecord(ev, s));
  return PCABO_OK;
}

// The single context's profile groups over those phases: 1 Normalize + Gram, 2 Cholesky, 3 root inverse + alpha (kk: the reduced
// dimension of group 1's work model).  Unprofiled, no event is recorded.
struct CondProf {
  pcabo_ctx* c; int kk;
  std::optional<ProfScope> ps;
  int operator()(int phase) {
    const double n = c->st.n;
    ps.reset();
    if (phase == 1) ps.emplace(c, 1, 8.0 * n * kk + 4.0 * n * (n + 1.0), 2.0 * n * n * kk + 12.0 * n * n);
    if (phase == 2) ps.emplace(c, 2, 16.0 * n * n, n * n * n / 3.0);
    if (phase == 3) ps.emplace(c, 3, 16.0 * n * n, n * n * n / 3.0 + 2.0 * n * n);
    return PCABO_OK;
  }
};

static int launch_factorisation(pcabo_ctx* ctx, double jitter) {
  hipStream_t s = ctx->stream;
  if (jitter > 0.0) {      // a retry: K is built again (same kernel, same bits, flag cleared), then the jitter goes on its diagonal
    launch_gram(s, ctx->dAT, ctx->dNrm, ctx->st.n, ctx->st.NP, round_up(ctx->st.k, 4), ctx->ld, ctx->st.noise, ctx->st.kernel, nullptr, nullptr,
                ctx->dL, ctx->dInfo);
    launch_add_jitter(s, ctx->dL, ctx->st.n, ctx->ld, jitter);
  }
  return enqueue_factor(ctx, s, ctx->st.n, ctx->st.NP, ZB(), CondProf{ctx, 0});
}

// psd_safe_cholesky's ladder for one context from `attempt` on (jitter 0, 1e-8, 1e-7, 1e-6).  Attempt 0 finds its factorisation
// already on the stream; a later one redoes it with that attempt's jitter.  Each attempt: extra() (launches the caller wants behind
// the factorisation; PCABO_OK or an error), one wait, the look at chol_info.  PCABO_OK, PCABO_ERR_NOT_PD or the launch / HIP error;
// either way the conditioning has ended, and the context's record is told how (ok with *used, the rung it ended on, or failed).
template <class Extra>
static int factor_ladder(pcabo_ctx* ctx, int attempt, Extra&& extra, double* used_out) {
  double jitter = 1e-8, &used = *used_out;
  for (int a = 2; a <= attempt; ++a) jitter *= 10.0;
  for (;; ++attempt) {
    if (attempt > 0) {
      const int rc = launch_factorisation(ctx, jitter);
      if (rc != PCABO_OK) return rc;
      used = jitter;
      jitter *= 10.0;
    }
    const int rc = extra();
    if (rc != PCABO_OK) return rc;
    HIPCHK(wait_stream(ctx->stream));
    HIPCHK(hipGetLastError());
    if (ctx->hm->chol_info == 0) return PCABO_OK;
    if (attempt == 3)
      return set_err(ctx, PCABO_ERR_NOT_PD, "K + s2 I not positive definite after jitter retries (pivot %s%d)", "", ctx->hm->chol_info);
  }
}
template <class Extra>
static int factor_attempts(pcabo_ctx* ctx, int attempt, Extra&& extra) {
  double used = 0.0;
  const int rc = factor_ladder(ctx, attempt, extra, &used);
  if (rc == PCABO_OK) ctx->st.condition_ended_ok(used);      // (pcabo_gp_extend borders K as it was factored: the rung is kept)
  else ctx->st.condition_failed();
  return rc;
}
static int factor_attempts(pcabo_ctx* ctx, int attempt) { return factor_attempts(ctx, attempt, [] { return (int)PCABO_OK; }); }

extern "C" {

int pcabo_ctx_create(int device, int max_n, int max_d, int max_q, pcabo_ctx** out) {
  if (!out) return PCABO_ERR_ARG;
  *out = nullptr;
  if (!ctx_sizes_ok(max_n, max_d, max_q)) return PCABO_ERR_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return PCABO_ERR_HIP;
  pcabo_ctx* ctx = new (std::nothrow) pcabo_ctx();
  if (!ctx) return PCABO_ERR_HIP;
  *out = ctx;                       // handed back even on failure so the caller can read the message
  return ctx_setup(ctx, device, ctx_layout(ctx_shape(max_n, max_d, max_q)), nullptr, nullptr, nullptr);
}

int pcabo_ctx_destroy(pcabo_ctx* ctx) {
  if (!ctx) return PCABO_ERR_ARG;
  if (ctx->in_batch) return set_err(ctx, PCABO_ERR_ARG, "pcabo_ctx_destroy: the context belongs to a batch (pcabo_batch_destroy frees it)%s", "");
  ctx_teardown(ctx);
  delete ctx;
  return PCABO_OK;
}

int pcabo_set_pointer_mode(pcabo_ctx* ctx, int mode) {
  if (!ctx || (mode != PCABO_PTR_HOST && mode != PCABO_PTR_DEVICE)) return PCABO_ERR_ARG;
  ctx->ptr_mode = mode;
  return PCABO_OK;
}

int pcabo_set_option(pcabo_ctx* ctx, int option, int value) {
  if (!ctx) return PCABO_ERR_ARG;
  switch (option) {
    case PCABO_OPT_RESIDENT: ctx->opt_resident = value != 0 && !ctx->in_batch; return PCABO_OK;   // (never inside a batch)
    case PCABO_OPT_BESTF_F32: ctx->bestf_f32 = value != 0; return PCABO_OK;
    case PCABO_OPT_GROUP_ACQ: ctx->opt_group_acq = value != 0; return PCABO_OK;
    case PCABO_OPT_HIDDEN_TAIL: ctx->opt_hidden_tail = value != 0; return PCABO_OK;
    default: return set_err(ctx, PCABO_ERR_ARG, "pcabo_set_option: unknown option %s%d", "", option);
  }
}

int pcabo_last_error(pcabo_ctx* ctx, char* buf, int buflen) {
  if (!ctx || !buf || buflen <= 0) return PCABO_ERR_ARG;
  snprintf(buf, buflen, "%s", ctx->err);
  return PCABO_OK;
}

// bulk input: copy host data to the staging buffer, or use the caller's device pointer as is
#define STAGE_IN(dst, src, count, T)                                                                        \
  do {                                                                                                      \
    if (ctx->ptr_mode == PCABO_PTR_HOST) {                                                                  \
      HIPCHK(hipMemcpyAsync((void*)(dst), (const void*)(src), (size_t)(count) * sizeof(T), hipMemcpyHostToDevice, ctx->stream)); \
    } else {                                                                                                \
      HIPCHK(hipMemcpyAsync((void*)(dst), (const void*)(src), (size_t)(count) * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream)); \
    }                                                                                                       \
  } while (0)
#define STAGE_OUT(dst, src, count, T)                                                                       \
  do {                                                                                                      \
    HIPCHK(hipMemcpyAsync((void*)(dst), (const void*)(src), (size_t)(count) * sizeof(T),                    \
                          ctx->ptr_mode == PCABO_PTR_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream)); \
  } while (0)
#define HOST_OUT(dst, src, count, T) \
  HIPCHK(hipMemcpyAsync((void*)(dst), (const void*)(src), (size_t)(count) * sizeof(T), hipMemcpyDeviceToHost, ctx->stream))

// ---- rows A-C (+ D-H behind them) ---------------------------------------------------------------------------------
// Inputs of one BO iteration.  Host-pointer mode: X, the noise block, the ranks (or f) and y are packed into one pinned
// buffer and cross in ONE copy (four pageable copies cost 60-170 us of host time per iteration); device-pointer mode:
// device-to-device copies into the context's own buffers as before.
static int stage_inputs(pcabo_ctx* ctx, const double* X, const double* f, const int64_t* ranks, const double* noise,
                        const double* y, int n, int d, int maximize, WpcaInputs* in) {
  hipStream_t s = ctx->stream;
  const size_t nd = (size_t)n * d;
  if (ctx->ptr_mode == PCABO_PTR_HOST) {
    double* h = ctx->hIn;
    const InPack pk = in_pack(n, d, noise != nullptr, true, y != nullptr);
    memcpy(h, X, nd * sizeof(double));                               in->X = ctx->dIn;
    if (noise) { memcpy(h + pk.noise, noise, nd * sizeof(double));   in->noise = ctx->dIn + pk.noise; }
    memcpy(h + pk.ranks, ranks ? (const void*)ranks : (const void*)f, (size_t)n * 8);
    if (y) { memcpy(h + pk.y, y, (size_t)n * sizeof(double));        in->y = ctx->dIn + pk.y; }
    // (segments are only 8-byte aligned: none of the consumers uses wider loads on them)
    HIPCHK(hipMemcpyAsync(ctx->dIn, h, pk.total * sizeof(double), hipMemcpyHostToDevice, s));
    if (ranks) in->ranks = (const long long*)(ctx->dIn + pk.ranks);
    else { launch_rank(s, ctx->dIn + pk.ranks, n, maximize, ctx->dRanks); in->ranks = ctx->dRanks; }
    return PCABO_OK;
  }
  STAGE_IN(ctx->dX, X, nd, double);                                  in->X = ctx->dX;
  if (ranks) { STAGE_IN(ctx->dRanks, ranks, n, long long); }
  else { STAGE_IN(ctx->dF, f, n, double); launch_rank(s, ctx->dF, n, maximize, ctx->dRanks); }
  in->ranks = ctx->dRanks;
  if (noise) { STAGE_IN(ctx->dNoise, noise, nd, double);             in->noise = ctx->dNoise; }
  if (y) { STAGE_IN(ctx->dY, y, n, double);                          in->y = ctx->dY; }
  return PCABO_OK;
}

// wPCA launches, then ONE copy of [data_mean | pca_mean | evr | comps] to pinned memory and the event that says it
// arrived.  k arrives through the HostMirror (written by the selection step at the end of k_jacobi).
static int enqueue_wpca(pcabo_ctx* ctx, const WpcaInputs& in, int n, int d, double var_threshold, int n_components) {
  std::optional<ProfScope> ps;
  return enqueue_rows_ac(ctx, ctx->stream, ctx->st, in, n, d, var_threshold, n_components, ZB(), ctx->evPca, [&](int behind) {
    if (behind) ps.reset();
    else ps.emplace(ctx, 0, 8.0 * n * d * 2 + 8.0 * n * d, 2.0 * n * d * d + 9.0 * d * d * d + 2.0 * n * d * d);
  });
}

// a run's wPCA results from its pinned block to the caller's arrays (null: not asked for)
static void wpca_hand_out(const pcabo_ctx* ctx, int d, int rcount, double* data_mean, double* pca_mean, double* comps, double* evr) {
  const double* h = small_at(ctx, small_wpca(ctx->lay.s));
  const PcaParts pp = pca_parts(ctx->lay.s);
  if (data_mean) memcpy(data_mean, h + pp.data_mean, (size_t)d * sizeof(double));
  if (pca_mean) memcpy(pca_mean, h + pp.pca_mean, (size_t)d * sizeof(double));
  if (evr) memcpy(evr, h + pp.evr, (size_t)rcount * sizeof(double));
  if (comps) memcpy(comps, h + pp.comps, (size_t)rcount * d * sizeof(double));
}

// wait for the results of the wPCA last enqueued only (whatever was enqueued behind them keeps running) and hand them out
static int collect_wpca(pcabo_ctx* ctx, double* data_mean, double* pca_mean, double* comps, double* evr, int* k) {
  HIPCHK(wait_event(ctx->evPca));
  HIPCHK(hipGetLastError());
  const int n = ctx->st.wpca_n, d = ctx->st.wpca_d;
  wpca_hand_out(ctx, d, n < d ? n : d, data_mean, pca_mean, comps, evr);
  ctx->st.wpca_collected(ctx->hm->k);
  if (k) *k = ctx->st.k;
  return PCABO_OK;
}
// ... where a call needs them and nobody has asked for them yet
static int collect_pending_wpca(pcabo_ctx* ctx) {
  return ctx->st.wpca_uncollected ? pcabo_wpca_results(ctx, nullptr, nullptr, nullptr, nullptr, nullptr) : PCABO_OK;
}

int pcabo_wpca(pcabo_ctx* ctx, const double* X, const double* f, const int64_t* ranks, int n, int d, int maximize,
               double var_threshold, int n_components, const double* noise, double* data_mean, double* pca_mean,
               double* comps, double* evr, int* k, double* Z) {
  if (!ctx) return PCABO_ERR_ARG;
  if (!X || (!f && !ranks) || n < 2 || n > ctx->max_n || d < 1 || d > ctx->max_d)
    return set_err(ctx, PCABO_ERR_ARG, "pcabo_wpca: bad argument or size beyond context capacity%s", "");
  if (ctx->st.in_flight()) return set_err(ctx, PCABO_ERR_ARG, "pcabo_wpca: a conditioning is in flight, call pcabo_gp_condition_end first%s", "");
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  WpcaInputs in{nullptr, nullptr, nullptr, nullptr};
  int rc = stage_inputs(ctx, X, f, ranks, noise, nullptr, n, d, maximize, &in);
  if (rc != PCABO_OK) return rc;
  rc = enqueue_wpca(ctx, in, n, d, var_threshold, n_components);
  if (rc != PCABO_OK) return rc;
  ctx->st.points_replaced(n);
  rc = collect_wpca(ctx, data_mean, pca_mean, comps, evr, k);
  if (rc != PCABO_OK) return rc;
  if (Z) {
    STAGE_OUT(Z, ctx->dZ, (size_t)n * ctx->st.k, double);
    HIPCHK(hipStreamSynchronize(s));
  }
  return PCABO_OK;
}

// Rows D-H on the stream, inputs on the device.  k < 0: the reduced dimension is still on its way (the launches sit
// right behind the wPCA) - the three kernels that need it read it from ctx->dK.
static int enqueue_condition(pcabo_ctx* ctx, const double* y_dev, int n, int k, const double* unb, double lengthscale,
                             double noise, int kernel, double mean_c = 0.0, const double* ard_ls = nullptr) {
  // (a profiled context keeps everything on one stream: its event pairs time the main stream alone)
  ctx->st.condition_enqueued(n, k, lengthscale, noise, kernel, ctx->stream2 && ctx->opt_hidden_tail && !ctx->prof);
  // the per-query tickets count modulo the number of slab groups: they only need a reset when that number changes
  // (every 64th iteration) or after a launch that did not complete
  const bool reset = ctx->st.tickets_reset_if_needed(acq_slabs(ctx->st.NP));
  const RowsDH a{ctx->dZ, y_dev, unb, n, k, ctx->st.KP, k < 0 ? ctx->dK : nullptr, 1.0 / lengthscale, noise, mean_c, kernel, ZB(),
                 {ctx->evBounds, nullptr}, reset, ard_ls, ctx->st.zn_recorded ? ctx->evZn : nullptr};
  return enqueue_rows_dh(ctx, ctx->stream, a, CondProf{ctx, k < 0 ? ctx->max_d : k});   // asynchronous: pcabo_gp_condition_end() waits and checks
}

// Z (or NULL: the projection a matching pcabo_wpca left in dZ), y and the user's Normalize bounds onto the device; *unb = the
// device copy of the bounds or NULL
static int stage_gp_inputs(pcabo_ctx* ctx, const double* Z, const double* y, int n, int k, const double* norm_bounds, const double** unb) {
  HIPCHK(hipSetDevice(ctx->device));
  if (Z) STAGE_IN(ctx->dZ, Z, (size_t)n * k, double);
  STAGE_IN(ctx->dY, y, n, double);
  *unb = nullptr;
  if (norm_bounds) {
    HIPCHK(hipMemcpyAsync(ctx->dUserNB, norm_bounds, (size_t)2 * k * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    *unb = ctx->dUserNB;
  }
  return PCABO_OK;
}

static bool gp_args_ok(const pcabo_ctx* ctx, int n, double lengthscale, double noise, int kernel) {
  return n >= 2 && n <= ctx->max_n && lengthscale > 0.0 && noise >= 0.0 &&
         (kernel == PCABO_KERNEL_MATERN52 || kernel == PCABO_KERNEL_RBF);
}

int pcabo_gp_condition_begin(pcabo_ctx* ctx, const double* Z, const double* y, int n, int k, const double* norm_bounds,
                             double lengthscale, double noise, int kernel) {
  if (!ctx) return PCABO_ERR_ARG;
  if (!y || k < 1 || k > ctx->max_d || !gp_args_ok(ctx, n, lengthscale, noise, kernel))
    return set_err(ctx, PCABO_ERR_ARG, "pcabo_gp_condition: bad argument or size beyond context capacity%s", "");
  if (!Z && !ctx->st.wpca_matches(n, k))
    return set_err(ctx, PCABO_ERR_ARG, "pcabo_gp_condition: Z == NULL needs a matching pcabo_wpca call first%s", "");
  const double* unb = nullptr;
  const int rc = stage_gp_inputs(ctx, Z, y, n, k, norm_bounds, &unb);
  if (rc != PCABO_OK) return rc;
  return enqueue_condition(ctx, ctx->dY, n, k, unb, lengthscale, noise, kernel);
}

// pcabo_wpca followed by pcabo_gp_condition_begin(Z = NULL, norm_bounds = NULL) as ONE enqueue: the conditioning
// launches go onto the stream right behind the projection, before the host has seen k, so the device does not idle
// while the wPCA results travel and the caller prepares the second call.  Returns as soon as the wPCA results are on
// the host; finish with pcabo_gp_condition_end().
int pcabo_wpca_gp_condition_begin(pcabo_ctx* ctx, const double* X, const double* f, const int64_t* ranks, int n, int d,
                                  int maximize, double var_threshold, int n_components, const double* noise,
                                  const double* y, double lengthscale, double gp_noise, int kernel, double* data_mean,
                                  double* pca_mean, double* comps, double* evr, int* k) {
  if (!ctx) return PCABO_ERR_ARG;
  if (!X || !y || (!f && !ranks) || d < 1 || d > ctx->max_d || !gp_args_ok(ctx, n, lengthscale, gp_noise, kernel))
    return set_err(ctx, PCABO_ERR_ARG, "pcabo_wpca_gp_condition_begin: bad argument or size beyond context capacity%s", "");
  if (ctx->st.in_flight()) return set_err(ctx, PCABO_ERR_ARG, "pcabo_wpca_gp_condition_begin: a conditioning is in flight, call pcabo_gp_condition_end first%s", "");
  HIPCHK(hipSetDevice(ctx->device));
  WpcaInputs in{nullptr, nullptr, nullptr, nullptr};
  int rc = stage_inputs(ctx, X, f, ranks, noise, y, n, d, maximize, &in);
  if (rc != PCABO_OK) return rc;
  rc = enqueue_wpca(ctx, in, n, d, var_threshold, n_components);
  if (rc != PCABO_OK) return rc;
  if (ctx->prof) {                       // profiled runs keep the two phases apart (the work model of group 1 needs k)
    rc = collect_wpca(ctx, data_mean, pca_mean, comps, evr, k);
    if (rc != PCABO_OK) return rc;
    return enqueue_condition(ctx, in.y, n, ctx->st.k, nullptr, lengthscale, gp_noise, kernel);
  }
  rc = enqueue_condition(ctx, in.y, n, -1, nullptr, lengthscale, gp_noise, kernel);      // (k on the device: the wPCA is uncollected)
  if (rc != PCABO_OK) return rc;
  if (!data_mean && !pca_mean && !comps && !evr && !k) return PCABO_OK;      // enqueue only: pcabo_wpca_results() waits
  return pcabo_wpca_results(ctx, data_mean, pca_mean, comps, evr, k);
}

// Second half of pcabo_wpca_gp_condition_begin when that was called without output pointers: waits for the wPCA
// results (the conditioning keeps running) and hands them out.  Lets the host do work that only needs a GUESS of k (the
// scrambled Sobol engine of the initial-condition draw, with last iteration's k) while the eigen-decomposition runs.
int pcabo_wpca_results(pcabo_ctx* ctx, double* data_mean, double* pca_mean, double* comps, double* evr, int* k) {
  if (!ctx) return PCABO_ERR_ARG;
  if (!ctx->st.wpca_known()) return set_err(ctx, PCABO_ERR_ARG, "pcabo_wpca_results: no weighted PCA enqueued%s", "");
  HIPCHK(hipSetDevice(ctx->device));
  return collect_wpca(ctx, data_mean, pca_mean, comps, evr, k);
}

int pcabo_gp_condition_end(pcabo_ctx* ctx) {
  if (!ctx) return PCABO_ERR_ARG;
  if (!ctx->st.in_flight()) return set_err(ctx, PCABO_ERR_ARG, "pcabo_gp_condition_end: no conditioning in flight%s", "");
  HIPCHK(hipSetDevice(ctx->device));
  if (const int rc = collect_pending_wpca(ctx)) return rc;
  return factor_attempts(ctx, 0);
}

int pcabo_gp_condition(pcabo_ctx* ctx, const double* Z, const double* y, int n, int k, const double* norm_bounds,
                       double lengthscale, double noise, int kernel) {
  int rc = pcabo_gp_condition_begin(ctx, Z, y, n, k, norm_bounds, lengthscale, noise, kernel);
  if (rc != PCABO_OK) return rc;
  return pcabo_gp_condition_end(ctx);
}

// ---- opt-in GP hyperparameter fit (DESIGN.md "GP hyperparameter fit") -------------------------------------------
// theta = {noise s2, mean constant c, rho_1 .. rho_m}: the shared lengthscale (m = 1) or, ard, one per input (m = k).  The host
// arithmetic of an evaluation (softplus_host, mll_theta_ok, mll_assemble) and the rules of a fit (FitRun, fit_rounds) are in
// host_side.h, shared by the single context and the batch.
static_assert(FIT_ARD_MAXVAR == 2 + PCABO_MAXD, "host_side.h sizes a run for PCABO_MAXD lengthscales");

// Inputs of a fit staged like pcabo_gp_condition_begin's; *unb = the device copy of the user's Normalize bounds or NULL.
static int stage_fit_inputs(pcabo_ctx* ctx, const char* who, bool ard, const double* Z, const double* y, int n, int k,
                            const double* norm_bounds, int kernel, const double** unb) {
  if (ard && ctx->in_batch) return set_err(ctx, PCABO_ERR_ARG, "%s: the context belongs to a batch (its ARD fit: pcabo_batch_gp_mll_ard / pcabo_batch_gp_fit_ard)", who);
  if (!y || k < 1 || k > ctx->max_d || n < 2 || n > ctx->max_n)
    return set_err(ctx, PCABO_ERR_ARG, "%s: bad argument or size beyond context capacity", who);
  if (kernel != PCABO_KERNEL_MATERN52)
    return set_err(ctx, PCABO_ERR_ARG, "%s: the fit is restated for the Matern-5/2 kernel only", who);
  if (ctx->st.in_flight()) return set_err(ctx, PCABO_ERR_ARG, "%s: a conditioning is in flight, call pcabo_gp_condition_end first", who);
  if (const int rc = collect_pending_wpca(ctx)) return rc;
  if (!Z && !ctx->st.wpca_matches(n, k))
    return set_err(ctx, PCABO_ERR_ARG, "%s: Z == NULL needs a matching pcabo_wpca call first", who);
  return stage_gp_inputs(ctx, Z, y, n, k, norm_bounds, unb);
}

// The attempts of one evaluation from `attempt` on (factor_attempts): each one runs the likelihood kernels behind its
// factorisation and copies their 5 + M results (M = 1, ard: M = KP) in front of its wait.  A run of a batch whose lock-step round
// failed enters at attempt 1.
static int mll_attempts(pcabo_ctx* ctx, int attempt, bool ard) {
  return factor_attempts(ctx, attempt, [ctx, ard]() -> int {
    const int M = ard ? ctx->st.KP : 1;
    double* out = ctx->dMll + mll_result(ctx->st.NP, M).start;
    launch_mll_grad(ctx->stream, ard, ctx->dR, ctx->dAT, ctx->dNrm, ctx->dAlpha, ctx->dL, ctx->dYs, ctx->st.n, ctx->st.NP, ctx->st.KP, ctx->ld, ctx->dMll, out);
    HOST_OUT(ctx->hMll, out, mll_result(ctx->st.NP, M).count, double);
    return PCABO_OK;
  });
}

// One evaluation at a theta inside the model's domain: the conditioning there (k_zstats with the mean constant -> k_znorm -> k_gram
// -> Cholesky -> root inverse -> alpha), then mll_attempts; the sums are left in ctx->hMll.
// ard (DESIGN.md "ARD lengthscales"): the lengthscales softplus(rho_c) go to the device and k_zstats folds them into the Normalize
// ranges, so the evaluation is the scalar one at lengthscale 1 on the folded ranges (the record's lengthscale is 1: the acquisition kernels
// read the folded bounds4 and need no change); k_mll_grad<true> adds the per-input sums.  The next conditioning call passes no
// lengthscales and returns to the unfolded model.
static int mll_launch(pcabo_ctx* ctx, bool ard, int n, int k, const double* unb, const double* theta) {
  if (ard) {
    for (int c = 0; c < k; ++c) ctx->hArdLs[c] = softplus_host(theta[2 + c]);    // (the last evaluation's copy has been waited for)
    HIPCHK(hipMemcpyAsync(ctx->dArdLs, ctx->hArdLs, (size_t)k * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  }
  const int rc = enqueue_condition(ctx, ctx->dY, n, k, unb, ard ? 1.0 : softplus_host(theta[2]), theta[0], PCABO_KERNEL_MATERN52,
                                   theta[1], ard ? ctx->dArdLs : nullptr);
  if (rc != PCABO_OK) return rc;
  return mll_attempts(ctx, 0, ard);      // (waits: the conditioning has ended when this returns)
}
// (the shared-lengthscale form names pcabo_gp_mll whichever entry point met the theta: its text since the first fit)
static int theta_domain_err(pcabo_ctx* ctx, const char* who, bool ard) {
  if (!ard) return set_err(ctx, PCABO_ERR_ARG, "pcabo_gp_mll: theta outside the model's domain (noise > 0, finite values)%s", "");
  return set_err(ctx, PCABO_ERR_ARG, "%s: theta outside the model's domain (noise > 0, lengthscales > 0, finite values)", who);
}

// pcabo_gp_mll / pcabo_gp_mll_ard
static int gp_mll_call(pcabo_ctx* ctx, const char* who, bool ard, const double* Z, const double* y, int n, int k,
                       const double* norm_bounds, int kernel, const double* theta, double* loss, double* grad) {
  if (!ctx) return PCABO_ERR_ARG;
  if (!theta || !loss) return set_err(ctx, PCABO_ERR_ARG, "%s: theta and loss are required", who);
  const double* unb = nullptr;
  int rc = stage_fit_inputs(ctx, who, ard, Z, y, n, k, norm_bounds, kernel, &unb);
  if (rc != PCABO_OK) return rc;
  const int m = ard ? k : 1;
  if (!mll_theta_ok(theta, m)) return theta_domain_err(ctx, who, ard);
  rc = mll_launch(ctx, ard, n, k, unb, theta);
  if (rc != PCABO_OK) return rc;
  mll_assemble(ctx->hMll, n, m, theta, loss, grad);
  return PCABO_OK;
}

// pcabo_gp_fit / pcabo_gp_fit_ard: scipy.optimize.minimize(method="L-BFGS-B") with its defaults around mll_launch: one FitRun,
// every round one evaluation.  The context is left conditioned at the result.
static int gp_fit_call(pcabo_ctx* ctx, const char* who, bool ard, const double* Z, const double* y, int n, int k,
                       const double* norm_bounds, int kernel, double* theta_inout, double* loss, int* info) {
  if (!ctx) return PCABO_ERR_ARG;
  if (!theta_inout) return set_err(ctx, PCABO_ERR_ARG, "%s: theta_inout is required", who);
  const double* unb = nullptr;
  int rc = stage_fit_inputs(ctx, who, ard, Z, y, n, k, norm_bounds, kernel, &unb);
  if (rc != PCABO_OK) return rc;
  std::vector<FitRun> run(1);
  run[0].init(theta_inout, ard ? k : 1, ard);
  run[0].bind(ctx->hMll);
  fit_rounds(run, n, [&](const std::vector<const double*>& th, int* st) { st[0] = mll_launch(ctx, ard, n, k, unb, th[0]); return (int)PCABO_OK; });
  const FitRun& r = run[0];
  if (r.status == PCABO_ERR_ARG) return theta_domain_err(ctx, who, ard);
  if (r.status != PCABO_OK) return r.status;
  memcpy(theta_inout, r.xr, (size_t)r.nvar * sizeof(double));
  if (loss) *loss = r.fr;
  if (info) r.report(info);
  return PCABO_OK;
}

int pcabo_gp_mll(pcabo_ctx* ctx, const double* Z, const double* y, int n, int k, const double* norm_bounds, int kernel,
                 const double* theta, double* loss, double* grad) {
  return gp_mll_call(ctx, "pcabo_gp_mll", false, Z, y, n, k, norm_bounds, kernel, theta, loss, grad);
}
int pcabo_gp_fit(pcabo_ctx* ctx, const double* Z, const double* y, int n, int k, const double* norm_bounds, int kernel,
                 double* theta_inout, double* loss, int* info) {
  return gp_fit_call(ctx, "pcabo_gp_fit", false, Z, y, n, k, norm_bounds, kernel, theta_inout, loss, info);
}
int pcabo_gp_mll_ard(pcabo_ctx* ctx, const double* Z, const double* y, int n, int k, const double* norm_bounds, int kernel,
                     const double* theta, double* loss, double* grad) {
  return gp_mll_call(ctx, "pcabo_gp_mll_ard", true, Z, y, n, k, norm_bounds, kernel, theta, loss, grad);
}
int pcabo_gp_fit_ard(pcabo_ctx* ctx, const double* Z, const double* y, int n, int k, const double* norm_bounds, int kernel,
                     double* theta_inout, double* loss, int* info) {
  return gp_fit_call(ctx, "pcabo_gp_fit_ard", true, Z, y, n, k, norm_bounds, kernel, theta_inout, loss, info);
}

int pcabo_acq_bounds(pcabo_ctx* ctx, double* bounds) {
  if (!ctx || !bounds) return PCABO_ERR_ARG;
  if (const int rc = collect_pending_wpca(ctx)) return rc;
  if (ctx->st.in_flight()) {                   // conditioning in flight: the box only needs k_zstats, wait for that alone
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(wait_event(ctx->evBounds));
  } else if (!ctx->st.conditioned()) {
    return set_err(ctx, PCABO_ERR_ARG, "pcabo_acq_bounds: call pcabo_gp_condition first%s", "");
  }
  for (int c = 0; c < ctx->st.k; ++c) { bounds[c] = ctx->hm->acq_lo[c]; bounds[ctx->st.k + c] = ctx->hm->acq_hi[c]; }
  return PCABO_OK;
}

// The one validity rule for (acq, scalar) of every acquisition entry point: a known PCABO_ACQ_* code and, for PCABO_ACQ_UCB,
// whose kappa = sqrt(beta) travels in the best_f slot, a finite kappa >= 0.  Null, or what is wrong.
static const char* acq_arg_error(int acq, double scalar) {
  if (acq != PCABO_ACQ_LOG_EI && acq != PCABO_ACQ_PI && acq != PCABO_ACQ_UCB) return "unknown acquisition code";
  if (acq == PCABO_ACQ_UCB && !(std::isfinite(scalar) && scalar >= 0.0))
    return "PCABO_ACQ_UCB takes kappa = sqrt(beta) in the best_f slot: it must be finite and >= 0";
  return nullptr;
}

static AcqParams make_params(pcabo_ctx* ctx, double best_f, int maximize, int acq, int want_grad) {
  AcqParams p;
  // torch.as_tensor(python float) gives a float32 tensor; a numpy float64 scalar keeps its 64 bits (PCABO_OPT_BESTF_F32);
  // PCABO_ACQ_UCB: the slot carries kappa, which the Python layer passes float32-representable already
  p.best_f = ctx->bestf_f32 ? (double)(float)best_f : best_f;
  p.y_mean = 0.0; p.y_std = 1.0;
  p.inv_ls = 1.0 / ctx->st.lengthscale;
  p.maximize = maximize ? 1 : 0;
  p.acq = acq;
  p.kernel = ctx->st.kernel;
  p.want_grad = want_grad;
  return p;
}

// the conditioned model of a context as the acquisition launchers take it
static GpModel gp_model(const pcabo_ctx* c) { return {c->st.n, c->st.k, c->st.NP, c->ld, c->dZnT, c->dR, c->dAlpha, c->dBounds4, c->dYstats}; }
static GpArrays gp_arrays(const pcabo_ctx* c) { return {c->dZnMean, c->dL, c->dR, c->dZnT, c->dAT, c->dNrm, c->dYs}; }

// The outcome of waiting for an acquisition launch's flags
static int acq_published(pcabo_ctx* ctx, FlagWait w) {
  if (w == FLAGS_UNPUBLISHED) {
    HIPCHK(hipGetLastError());
    return set_err(ctx, PCABO_ERR_TIMEOUT, "acquisition kernel finished without publishing its results%s", "");
  }
  if (w == FLAGS_LATE) return set_err(ctx, PCABO_ERR_TIMEOUT, "device did not publish acquisition results%s", "");
  return PCABO_OK;
}

// Host work that needs no result of the device: done once, where everything of an evaluation is enqueued and its wait has not
// begun (pcabo_propose_acqf draws the variates of its pick there).  An evaluation that is repeated does not repeat it.
struct HostWork {
  std::function<void()> fn;
  void run() { if (fn) { fn(); fn = nullptr; } }
};
static void run_beside(HostWork* w) { if (w) w->run(); }

// One evaluation of the acquisition at the nq points staged in ctx->hXq (pinned): a single fused launch
// whose results land in ctx->hVal / ctx->hGrad; the host spins on the sequence flag.
static int eval_staged(pcabo_ctx* ctx, int nq, AcqParams& p, bool allow_gemm = true, HostWork* beside = nullptr) {
  hipStream_t s = ctx->stream;
  const int k = ctx->st.k;
  const unsigned long long seq = ++ctx->seq;
  const QueryArgs* qa = nullptr;
  const double* xdev = nullptr;
  if ((size_t)nq * k <= PCABO_QA_MAX) {
    qa = reinterpret_cast<const QueryArgs*>(ctx->hXq);        // copied by value into the kernel arguments
  } else {
    HIPCHK(hipMemcpyAsync(ctx->dXq, ctx->hXq, (size_t)nq * k * sizeof(double), hipMemcpyHostToDevice, s));
    xdev = ctx->dXq;
  }
  const bool small = nq <= PCABO_INLAUNCH_MAXQ;   // in-launch combine + host flag; larger batches: two launches + copy
  if (!small && !p.want_grad && allow_gemm && score_gemm_possible(nq)) {
    // value-only scoring of a large batch (the raw samples): V = R KS^T on MFMA
    if (!xdev) {
      HIPCHK(hipMemcpyAsync(ctx->dXq, ctx->hXq, (size_t)nq * k * sizeof(double), hipMemcpyHostToDevice, s));
      xdev = ctx->dXq;
    }
    ProfScope ps(ctx, 5, acq_bytes(ctx->st.n, k, nq, 0), acq_flops(ctx->st.n, k, nq, 0));
    launch_score(s, xdev, nq, gp_model(ctx), p, ctx->dKS, ctx->dPartial, ctx->dVal);
  } else {
    ProfScope ps(ctx, small ? 4 : 5, acq_bytes(ctx->st.n, k, nq, p.want_grad), acq_flops(ctx->st.n, k, nq, p.want_grad));
    launch_acq(s, qa, xdev, nq, gp_model(ctx), p, ctx->dPartial, ctx->dCounters, ctx->dVal, ctx->dGrad, small ? ctx->hVal : nullptr,
               small ? ctx->hGrad : nullptr, small ? ctx->hm : nullptr, seq);
  }
  if (!small) {
    HIPCHK(hipMemcpyAsync(ctx->hVal, ctx->dVal, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost, s));
    if (p.want_grad) HIPCHK(hipMemcpyAsync(ctx->hGrad, ctx->dGrad, (size_t)nq * k * sizeof(double), hipMemcpyDeviceToHost, s));
    run_beside(beside);
    HIPCHK(wait_stream(s));
    HIPCHK(hipGetLastError());
    return PCABO_OK;
  }
  run_beside(beside);
  return acq_published(ctx, wait_flags(ctx->hm, 0, nq, seq, deadline_in(20), &s));
}

// The part of the GEMM scoring that needs alpha and R, for nq samples whose kernel vectors are in ctx->dKS: the mu_s sums, V = R KS^T,
// the scalar chain per sample, the values' copy and the wait (eval_staged's GEMM branch without its first kernel's KS half).
static int score_tail(pcabo_ctx* ctx, int nq, AcqParams& p, HostWork* beside = nullptr) {
  hipStream_t s = ctx->stream;
  launch_score_tail(s, nq, gp_model(ctx), p, ctx->dKS, ctx->dPartial, ctx->dVal);
  HIPCHK(hipMemcpyAsync(ctx->hVal, ctx->dVal, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost, s));
  run_beside(beside);
  HIPCHK(wait_stream(s));
  HIPCHK(hipGetLastError());
  return PCABO_OK;
}

// The same for restart groups through the throughput kernel (PCABO_OPT_GROUP_ACQ): group g = the gn[g] <= 5 points staged
// at query slots g0[g].. of ctx->hXq, which the kernel reads in place (pinned memory); one work-group per (group, 64-row slab).
struct GroupLaunches {                   // at most 8 groups: PCABO_INLAUNCH_MAXQ queries in fives, or the restart groups of a call
  int g0[8], gn[8], ng = 0;
  void add(int q0, int n) { g0[ng] = q0; gn[ng] = n; ++ng; }
};
static int eval_staged_groups(pcabo_ctx* ctx, const GroupLaunches& t, AcqParams& p) {
  hipStream_t s = ctx->stream;
  const unsigned long long seq = ++ctx->seq;
  const int *g0 = t.g0, *gn = t.gn, ng = t.ng;
  QueryArgs tab;
  unsigned* ent = reinterpret_cast<unsigned*>(tab.x);
  for (int g = 0; g < ng; ++g) ent[g] = ((unsigned)g0[g] << 8) | (unsigned)gn[g];
  {
    int nq = 0;
    for (int g = 0; g < ng; ++g) nq += gn[g];
    ProfScope ps(ctx, 4, acq_bytes(ctx->st.n, ctx->st.k, nq, p.want_grad), acq_flops(ctx->st.n, ctx->st.k, nq, p.want_grad));
    if (launch_acq_group(s, &tab, ng, ctx->hXq, gp_model(ctx), p, ctx->dPartial, ctx->dCounters + counters_group().start, ctx->dVal,
                         ctx->dGrad, ctx->hVal, ctx->hGrad, ctx->hm, seq, AcqBatch()) != 0)
      return set_err(ctx, PCABO_ERR_HIP, "the restart-group acquisition kernel could not be launched%s", "");
  }
  HIPCHK(hipGetLastError());
  const auto deadline = deadline_in(20);
  FlagWait w = FLAGS_SET;
  for (int g = 0; g < ng && w == FLAGS_SET; ++g) w = wait_flags(ctx->hm, g0[g], gn[g], seq, deadline, &s);
  return acq_published(ctx, w);
}
static bool group_mode(const pcabo_ctx* ctx, int q, int want_grad) {
  return ctx->opt_group_acq && want_grad && q <= PCABO_INLAUNCH_MAXQ && acq_group_possible(ctx->st.NP, ctx->st.k);
}

// The values of the acquisition at the q host points Xq on the conditioned model, into ctx->hVal: pcabo_acq_eval without a gradient
// on host pointers, behind its checks.
static int values_staged(pcabo_ctx* ctx, const double* Xq, int q, double best_f, int maximize, int acq, HostWork* beside = nullptr) {
  HIPCHK(hipSetDevice(ctx->device));
  memcpy(ctx->hXq, Xq, (size_t)q * ctx->st.k * sizeof(double));
  AcqParams p = make_params(ctx, best_f, maximize, acq, 0);
  return eval_staged(ctx, q, p, true, beside);
}

int pcabo_acq_eval(pcabo_ctx* ctx, const double* Xq, int q, double best_f, int maximize, int acq, double* val,
                   double* grad) {
  if (!ctx) return PCABO_ERR_ARG;
  if (!Xq || !val || q < 1 || q > ctx->max_q)
    return set_err(ctx, PCABO_ERR_ARG, "pcabo_acq_eval: bad argument or q beyond context capacity%s", "");
  if (const char* why = acq_arg_error(acq, best_f)) return set_err(ctx, PCABO_ERR_ARG, "pcabo_acq_eval: %s", why);
  if (!ctx->st.conditioned()) return set_err(ctx, PCABO_ERR_ARG, "pcabo_acq_eval: call pcabo_gp_condition first%s", "");
  if (!grad && ctx->ptr_mode == PCABO_PTR_HOST) {
    const int rc = values_staged(ctx, Xq, q, best_f, maximize, acq);
    if (rc == PCABO_OK) memcpy(val, ctx->hVal, (size_t)q * sizeof(double));
    return rc;
  }
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int k = ctx->st.k;
  const size_t nx = (size_t)q * k;
  if (ctx->ptr_mode == PCABO_PTR_HOST) memcpy(ctx->hXq, Xq, nx * sizeof(double));
  else {
    HIPCHK(hipMemcpyAsync(ctx->hXq, Xq, nx * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  AcqParams p = make_params(ctx, best_f, maximize, acq, grad ? 1 : 0);
  int rc;
  if (group_mode(ctx, q, grad != nullptr) && ctx->ptr_mode == PCABO_PTR_HOST) {
    static_assert((PCABO_INLAUNCH_MAXQ + PCABO_GROUP_Q - 1) / PCABO_GROUP_Q <= 8, "GroupLaunches holds 8 groups");
    GroupLaunches t;
    for (int a = 0; a < q; a += PCABO_GROUP_Q) t.add(a, std::min(PCABO_GROUP_Q, q - a));
    rc = eval_staged_groups(ctx, t, p);
  } else {
    rc = eval_staged(ctx, q, p);
  }
  if (rc != PCABO_OK) return rc;
  if (ctx->ptr_mode == PCABO_PTR_HOST) {
    memcpy(val, ctx->hVal, (size_t)q * sizeof(double));
    if (grad) memcpy(grad, ctx->hGrad, nx * sizeof(double));
  } else {
    HIPCHK(hipMemcpyAsync(val, ctx->dVal, (size_t)q * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (grad) HIPCHK(hipMemcpyAsync(grad, ctx->dGrad, nx * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  return PCABO_OK;
}

// pcabo_gp_condition_end + pcabo_acq_eval (values only) with the evaluation ENQUEUED BEHIND the conditioning: the raw
// samples of the initial-condition draw are known before the factorisation has finished, so their copy and launches
// need not wait for the host to see it end.  If the factorisation turns out to have needed jitter, the values are
// computed again after the retries.
// ... behind its checks, on host pointers: the values land in ctx->hVal and the conditioning is over.
static int end_eval_staged(pcabo_ctx* ctx, const double* Xq, int q, double best_f, int maximize, int acq, HostWork* beside = nullptr) {
  if (const int rc = collect_pending_wpca(ctx)) return rc;
  if (q <= PCABO_INLAUNCH_MAXQ) {                    // nothing to gain: the two calls in a row
    run_beside(beside);
    const int rc = pcabo_gp_condition_end(ctx);
    return rc != PCABO_OK ? rc : values_staged(ctx, Xq, q, best_f, maximize, acq);
  }
  HIPCHK(hipSetDevice(ctx->device));
  memcpy(ctx->hXq, Xq, (size_t)q * ctx->st.k * sizeof(double));
  AcqParams p = make_params(ctx, best_f, maximize, acq, 0);
  // The kernel vectors of the samples need the Normalize bounds and ZnT only: they and the samples' copy go to the second stream
  // and run beside the factorisation; what needs alpha and R follows on the main stream (score_tail).
  const bool hidden = ctx->st.zn_consumed() && ctx->opt_hidden_tail && !ctx->prof && score_gemm_possible(q);
  int rc;
  if (hidden) {
    HIPCHK(hipStreamWaitEvent(ctx->stream2, ctx->evZn, 0));
    HIPCHK(hipMemcpyAsync(ctx->dXq, ctx->hXq, (size_t)q * ctx->st.k * sizeof(double), hipMemcpyHostToDevice, ctx->stream2));
    launch_score_ks_only(ctx->stream2, ctx->dXq, q, gp_model(ctx), p, ctx->dKS);
    HIPCHK(hipEventRecord(ctx->evKS, ctx->stream2));
    HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->evKS, 0));
    rc = score_tail(ctx, q, p, beside);
  } else {
    rc = eval_staged(ctx, q, p, true, beside);      // ends with a stream synchronisation: the conditioning is over too
  }
  if (rc != PCABO_OK) { ctx->st.condition_failed(); return rc; }
  if (ctx->hm->chol_info != 0) {                    // rare: jitter retries, then the evaluation again
    rc = pcabo_gp_condition_end(ctx);
    if (rc != PCABO_OK) return rc;
    // (K + jitter I changes R and alpha, not the kernel vectors: only the launches behind them run again)
    rc = hidden ? score_tail(ctx, q, p) : eval_staged(ctx, q, p);
    if (rc != PCABO_OK) return rc;
  } else {
    ctx->st.condition_ended_ok(0.0);                // (the factorisation as enqueued: no jitter)
  }
  return PCABO_OK;
}

int pcabo_gp_condition_end_eval(pcabo_ctx* ctx, const double* Xq, int q, double best_f, int maximize, int acq,
                                double* val) {
  if (!ctx) return PCABO_ERR_ARG;
  if (!Xq || !val || q < 1 || q > ctx->max_q)
    return set_err(ctx, PCABO_ERR_ARG, "pcabo_gp_condition_end_eval: bad argument or q beyond context capacity%s", "");
  if (const char* why = acq_arg_error(acq, best_f)) return set_err(ctx, PCABO_ERR_ARG, "pcabo_gp_condition_end_eval: %s", why);
  if (!ctx->st.in_flight()) return set_err(ctx, PCABO_ERR_ARG, "pcabo_gp_condition_end_eval: no conditioning in flight%s", "");
  if (ctx->ptr_mode != PCABO_PTR_HOST) {             // nothing to gain: the two calls in a row
    if (const int rc = collect_pending_wpca(ctx)) return rc;
    int rc = pcabo_gp_condition_end(ctx);
    if (rc != PCABO_OK) return rc;
    return pcabo_acq_eval(ctx, Xq, q, best_f, maximize, acq, val, nullptr);
  }
  const int rc = end_eval_staged(ctx, Xq, q, best_f, maximize, acq);
  if (rc == PCABO_OK) memcpy(val, ctx->hVal, (size_t)q * sizeof(double));
  return rc;
}

int pcabo_logei(pcabo_ctx* ctx, const double* Xq, int q, double best_f, int maximize, double* val, double* grad) {
  return pcabo_acq_eval(ctx, Xq, q, best_f, maximize, PCABO_ACQ_LOG_EI, val, grad);
}

// ---- resident acquisition kernel: host side of the mailbox ---------------------------------------------------------
// The mailbox of a resident kernel of `cap` queries, in device memory, written through the PCIe BAR: cap k coordinate pairs
// behind the first pair, then one control pair per query (1 = evaluate, 0 = leave for good).  A pair leaves in one 16-byte
// store and its tag is mixed with the value's bits (mail_mix), so a reader never takes a value that does not belong to its
// tag.  The kernel answers query q by its results in pinned host memory and then the tag in hm->qflag[q].
struct BarMailbox {
  MailPair* m; const HostMirror* hm; int cap, k;
  void coords(int q0, int nq, const double* x, unsigned long long tag) const {
    for (int t = 0; t < nq * k; ++t) put_mail_pair(m + 1 + q0 * k + t, x[t], tag);
  }
  void controls(int q0, int nq, double what, unsigned long long tag) const {
    for (int j = 0; j < nq; ++j) put_mail_pair(m + 1 + cap * k + q0 + j, what, tag);
  }
  void flush() const { _mm_sfence(); }   // the write-combining buffers leave now
  // the mailbox of free_pair (host_side.h): a group's own slots
  void post(int q0, int nq, const double* x, unsigned long long tag) const { coords(q0, nq, x, tag); controls(q0, nq, 1.0, tag); flush(); }
  unsigned long long tag_of(int q) const { return __atomic_load_n(&hm->qflag[q], __ATOMIC_ACQUIRE); }
  void leave(int q0, int nq, unsigned long long tag) const { controls(q0, nq, 0.0, tag); flush(); }
  // one lock-step round: all cap k coordinate pairs get the round's tag (coordinates of queries that are no longer active are
  // whatever is left in xq), the first nq queries are evaluated, the others leave
  void post_round(int nq, const double* xq, unsigned long long tag) const {
    coords(0, cap, xq, tag); controls(0, nq, 1.0, tag); controls(nq, cap - nq, 0.0, tag); flush();
  }
};

// The resident kernel of ONE optimise call: a launch of `cap` queries that stays on the chip and takes the evaluations of the call
// through the mailbox (see k_acq_fast): no launch and no operand refill per round.  Whatever way the call is left, the kernel is
// told to go and waited for (stop, the destructor).
struct ResidentSession {
  pcabo_ctx* ctx; AcqParams& p;
  int cap = 0;                           // > 0 while a kernel of that many queries is in flight
  BarMailbox mail() const { return BarMailbox{ctx->dMail, ctx->hm, cap, ctx->st.k}; }
  // Does this call, at its first round of nq queries, go to a resident kernel?  Only a process alone on the device, and only
  // the one context of it: several contexts in ONE process (one run per host thread, or a batch next to a single run) would
  // each want most of the chip at the same time - one launch per evaluation then, which interleaves well.  A call under a
  // penalty (the GPU looked shared, see round and free_pair) pays one unit of it and takes plain launches.
  bool wanted(unsigned round_no, int nq) {
    if (round_no != 1) return false;
    if ((ctx->alone_age++ & 7) == 0) ctx->alone = presence_alone(ctx->device);
    if (ctx->srv_penalty > 0) { --ctx->srv_penalty; return false; }
    return ctx->opt_resident && ctx->mail_bar && !ctx->opt_group_acq && ctx->alone && presence_local_contexts(ctx->device) == 1 &&
           !ctx->prof && acq_server_possible(nq, ctx->st.n, ctx->st.k, ctx->st.NP);
  }
  int start(int nq) {
    cap = nq;
    launch_acq(ctx->stream, nullptr, nullptr, cap, gp_model(ctx), p, ctx->dPartial, ctx->dCounters, ctx->dVal, ctx->dGrad,
               ctx->hVal, ctx->hGrad, ctx->hm, ctx->seq + 1, ctx->dMail, ctx->dPairs);
    HIPCHK(hipGetLastError());
    return PCABO_OK;
  }
  // One lock-step round of nq queries staged in ctx->hXq.  No answer within 3 s (e.g. this thread lost the CPU for longer than
  // the kernel waits): plain launches from here on.  A FIRST answer after more than a millisecond (normal: ~20 us) means the
  // grid could not become resident at once: another process holds the GPU with its own resident kernel.  Resident kernels of
  // different processes then run one after the other, whole calls at a time; plain launches interleave much better, so use
  // them for a while.
  int round(int nq, bool first) {
    const auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const unsigned long long tag = ++ctx->seq;
    const double tp = now();
    mail().post_round(nq, ctx->hXq, tag);
    if (wait_flags(ctx->hm, 0, nq, tag, deadline_in(3)) != FLAGS_SET) {
      (void)set_err(ctx, PCABO_ERR_TIMEOUT, "resident acquisition kernel did not answer%s", "");   // (the tickets may be dirty)
      stop();
      ctx->srv_penalty = 1000;
      return eval_staged(ctx, nq, p);
    }
    if (first && now() - tp > 1e-3) ctx->srv_penalty = 40;
    return PCABO_OK;
  }
  // The call's two groups free of each other (free_pair, host_side.h) until both have left the kernel, which ends with them.
  // A group that was not answered leaves the call to plain launches, and the next calls too.
  int pair(CrewCall& crew, RunRestarts& run) {
    const unsigned long long seq0 = ctx->seq;
    BarMailbox mb = mail();
    const FreePair fp = free_pair(crew, run, mb, seq0);
    HIPCHK(hipStreamSynchronize(ctx->stream));        // every group of the grid has been told to leave
    ctx->seq = seq0 + std::max(fp.used[0], fp.used[1]) + 1;
    cap = 0;
    if (fp.got_nan[0] || fp.got_nan[1]) return set_err(ctx, PCABO_ERR_NAN, "NaN in acquisition gradient%s", "");
    if (fp.timed_out[0] || fp.timed_out[1]) ctx->srv_penalty = 1000;
    else if (fp.slow_first[0] || fp.slow_first[1]) ctx->srv_penalty = 40;
    return PCABO_OK;
  }
  void stop() {
    if (cap <= 0) return;
    mail().post_round(0, ctx->hXq, ++ctx->seq);
    (void)hipStreamSynchronize(ctx->stream);
    cap = 0;
  }
  ~ResidentSession() { stop(); }
};

// ---- multi-start L-BFGS-B over the device acquisition ------------------------------------------
// All restart groups advance in lock-step: per round every still-active group asks for one joint value+gradient evaluation
// (CrewCall, host_side.h: the groups are stepped by up to seven threads); the points of all groups go to the device together
// (pack_active) and the results land in pinned host memory.  A round is evaluated by the call's resident kernel when it has one
// (two groups: free of each other from there on, free_pair), else by one launch: of k_acq_group per restart group
// (PCABO_OPT_GROUP_ACQ) or of the per-query kernels (eval_staged above).
static int optimize_checked(pcabo_ctx* ctx, const double* ics, int num_restarts, int batch_limit, const double* bounds, int maxiter,
                            double best_f, int maximize, int acq, double* cand, double* vals, int* info, int* failed);

int pcabo_optimize_acqf(pcabo_ctx* ctx, const double* ics, int num_restarts, int batch_limit, const double* bounds,
                        int maxiter, double best_f, int maximize, int acq, double* cand, double* vals, int* info,
                        int* failed) {
  if (!ctx) return PCABO_ERR_ARG;
  if (!ics || !bounds || !cand || !vals || num_restarts < 1 || batch_limit < 1 || num_restarts > ctx->max_q)
    return set_err(ctx, PCABO_ERR_ARG, "pcabo_optimize_acqf: bad argument%s", "");
  if (const char* why = acq_arg_error(acq, best_f)) return set_err(ctx, PCABO_ERR_ARG, "pcabo_optimize_acqf: %s", why);
  if (!ctx->st.conditioned()) return set_err(ctx, PCABO_ERR_ARG, "pcabo_optimize_acqf: call pcabo_gp_condition first%s", "");
  return optimize_checked(ctx, ics, num_restarts, batch_limit, bounds, maxiter, best_f, maximize, acq, cand, vals, info, failed);
}

// ... behind its checks (pcabo_propose_acqf comes here with the initial conditions it picked itself)
static int optimize_checked(pcabo_ctx* ctx, const double* ics, int num_restarts, int batch_limit, const double* bounds, int maxiter,
                            double best_f, int maximize, int acq, double* cand, double* vals, int* info, int* failed) {
  HIPCHK(hipSetDevice(ctx->device));
  const int k = ctx->st.k;
  RunRestarts run;
  run.init(ics, bounds, num_restarts, batch_limit, k, maxiter);
  run.bind(ctx->hXq, ctx->hVal, ctx->hGrad);
  std::vector<RestartGroup>& grp = run.grp;
  const int ngroups = (int)grp.size();
  AcqParams p = make_params(ctx, best_f, maximize, acq, 1);
  std::vector<char> pending(ngroups, 0);
  std::vector<int> qoff(ngroups, -1);
  CrewCall crew(ctx->crew, run, pending);
  ResidentSession srv{ctx, p};
  for (unsigned round_no = 1;; ++round_no) {
    if (round_no == 1) {                 // (clocked: what stands in front of the first round, the helper's wake-up included)
      const auto t = std::chrono::steady_clock::now();
      crew.advance_all();
      ctx->first_advance_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count();
    } else {
      crew.advance_all();
    }
    const int nq = pack_active(run, qoff);
    if (nq == 0) break;
    int rc;
    if (srv.wanted(round_no, nq)) {
      if ((rc = srv.start(nq)) != PCABO_OK) return rc;
      if (ngroups == 2 && grp[0].active && grp[1].active && nq == num_restarts) {
        if ((rc = srv.pair(crew, run)) != PCABO_OK) return rc;
        if (!grp[0].active && !grp[1].active) break;    // the normal end: both groups ran to their stop
        continue;                                       // a wait failed: the lock-step rounds finish the call
      }
    }
    if (srv.cap > 0) {
      rc = srv.round(nq, round_no == 1);
    } else if (group_mode(ctx, nq, 1) && batch_limit <= PCABO_GROUP_Q && ngroups <= 8) {
      GroupLaunches t;
      for (int gi = 0; gi < ngroups; ++gi) if (qoff[gi] >= 0) t.add(qoff[gi], grp[gi].nq);
      rc = eval_staged_groups(ctx, t, p);
    } else {
      rc = eval_staged(ctx, nq, p);
    }
    if (rc != PCABO_OK) return rc;
    if (!absorb_packed(run, qoff)) return set_err(ctx, PCABO_ERR_NAN, "NaN in acquisition gradient%s", "");
  }
  srv.stop();
  // botorch evaluates the acquisition once more at the clamped end points.  An L-BFGS-B run normally ends ON the last point
  // it had evaluated (the accepted trial of its last line search), whose per-restart values are still here - the same
  // kernel arithmetic, so the same bits; only a run that ended elsewhere (abnormal line search) needs the launch.
  const bool redo = run.end_points(cand, vals) > 0;
  const bool any_failed = run.report(info, 0);
  if (redo) {
    AcqParams pv = make_params(ctx, best_f, maximize, acq, 0);
    // (through the slab kernels whatever the number of restarts: the values of a restart must not depend on how many
    // restarts share the call)
    memcpy(ctx->hXq, cand, (size_t)num_restarts * k * sizeof(double));
    int rc = eval_staged(ctx, num_restarts, pv, false);
    if (rc != PCABO_OK) return rc;
    for (int j = 0; j < num_restarts; ++j) vals[j] = ctx->hVal[j];
  }
  if (failed) *failed = any_failed;
  return PCABO_OK;
}

// Rows K-N of a single run in one call: the raw samples are scored (behind the conditioning, if one is in flight), botorch's
// initialize_q_batch picks the initial conditions on the caller's generator blob, and the optimiser starts from them.  Between
// the scores and the optimiser's first round the host does only what needs the scores: the variates of the pick are drawn while
// it would otherwise wait for the device, and the stepping helper has left its condition variable by then.
int pcabo_propose_acqf(pcabo_ctx* ctx, const double* raw, int n_raw, void* blob, double eta, int num_restarts, int batch_limit,
                       const double* bounds, int maxiter, double best_f, int maximize, int acq, int flags, double* raw_vals,
                       int64_t* ic_idx, double* ics, double* cand, double* vals, int* info, int* failed, int* picked,
                       double* phase_seconds) {
  using clk = std::chrono::steady_clock;
  if (!ctx) return PCABO_ERR_ARG;
  if (!raw || !raw_vals || n_raw < 1 || n_raw > ctx->max_q)
    return set_err(ctx, PCABO_ERR_ARG, "pcabo_propose_acqf: bad argument or q beyond context capacity%s", "");
  if (!blob || !ic_idx || !ics || !picked || !bounds || !cand || !vals || num_restarts < 1 || batch_limit < 1 ||
      num_restarts > ctx->max_q || (flags & ~PCABO_PROPOSE_NO_WAKE))
    return set_err(ctx, PCABO_ERR_ARG, "pcabo_propose_acqf: bad argument%s", "");
  if (n_raw < 2 || num_restarts >= n_raw)
    return set_err(ctx, PCABO_ERR_ARG, "pcabo_propose_acqf: the pick takes fewer restarts than raw samples, of at least two%s", "");
  if (const char* why = acq_arg_error(acq, best_f)) return set_err(ctx, PCABO_ERR_ARG, "pcabo_propose_acqf: %s", why);
  if (acq == PCABO_ACQ_PI)
    return set_err(ctx, PCABO_ERR_ARG, "pcabo_propose_acqf: the pick of PCABO_ACQ_PI (botorch's non-negative variant) is the caller's%s", "");
  if (!torch_blob_ok(blob))
    return set_err(ctx, PCABO_ERR_ARG, "pcabo_propose_acqf: not a state blob of torch's CPU generator%s", "");
  if (ctx->ptr_mode != PCABO_PTR_HOST) return set_err(ctx, PCABO_ERR_ARG, "pcabo_propose_acqf: host pointers only%s", "");
  const bool pending = ctx->st.in_flight();
  if (!pending && !ctx->st.conditioned())
    return set_err(ctx, PCABO_ERR_ARG, "pcabo_propose_acqf: call pcabo_gp_condition first%s", "");
  *picked = 0;
  const auto t0 = clk::now();
  const auto since = [](clk::time_point a) { return std::chrono::duration<double>(clk::now() - a).count(); };
  double clocks[3] = {0.0, 0.0, 0.0};
  const auto hand_clocks = [&] { if (phase_seconds) std::copy(clocks, clocks + 3, phase_seconds); };
  std::unique_ptr<OptCrew::Awake> awake;
  if (!(flags & PCABO_PROPOSE_NO_WAKE) && num_restarts > batch_limit) awake.reset(new OptCrew::Awake(ctx->crew));
  // the variates of the pick need no score: drawn where the scoring is enqueued and its wait has not begun
  AheadPick ahead(n_raw, num_restarts);
  HostWork draw{[&] { ahead.draw(blob); }};
  int rc = pending ? end_eval_staged(ctx, raw, n_raw, best_f, maximize, acq, &draw)
                   : values_staged(ctx, raw, n_raw, best_f, maximize, acq, &draw);
  if (rc != PCABO_OK) {
    ahead.put_back();
    return rc;
  }
  draw.run();                                       // (a path that had no place for it)
  memcpy(raw_vals, ctx->hVal, (size_t)n_raw * sizeof(double));
  clocks[0] = since(t0);
  const auto t1 = clk::now();
  if (ahead.pick(raw_vals, eta, ic_idx) != 0) {     // no spread in the scores (the blob is back): botorch's other paths, in the caller
    clocks[1] = since(t1);
    hand_clocks();
    return PCABO_OK;
  }
  const int k = ctx->st.k;
  for (int j = 0; j < num_restarts; ++j) memcpy(ics + (size_t)j * k, raw + (size_t)ic_idx[j] * k, (size_t)k * sizeof(double));
  *picked = 1;
  clocks[1] = since(t1);
  const auto t2 = clk::now();
  rc = optimize_checked(ctx, ics, num_restarts, batch_limit, bounds, maxiter, best_f, maximize, acq, cand, vals, info, failed);
  clocks[2] = since(t2);
  hand_clocks();
  return rc;
}

// Debug export, not part of the ABI in include/pcabo.h (tools/gpu_propose_clock.py): the host time of the first advance_all of the
// context's last pcabo_optimize_acqf / pcabo_propose_acqf - every group's first L-BFGS-B step, behind the helper's wake-up.
double pcabo_debug_first_advance_seconds(pcabo_ctx* ctx) { return ctx ? ctx->first_advance_s : -1.0; }

int pcabo_inverse_map(pcabo_ctx* ctx, const double* z, double* x) {
  if (!ctx || !z || !x) return PCABO_ERR_ARG;
  if (!ctx->st.have_wpca) return set_err(ctx, PCABO_ERR_ARG, "pcabo_inverse_map: call pcabo_wpca first%s", "");
  if (!ctx->in_batch && ctx->opt_hidden_tail) {
    // A single context has [data_mean | pca_mean | evr | comps] in pinned host memory since the wPCA results were collected:
    // the k d multiply-adds run here, with the kernel's bits (inverse_map_host) - no launch, no flag wait, no device copy of x.
    if (const int rc = collect_pending_wpca(ctx)) return rc;
    const double* h = small_at(ctx, small_wpca(ctx->lay.s));
    const PcaParts pp = pca_parts(ctx->lay.s);
    inverse_map_host(z, h + pp.comps, h + pp.pca_mean, h + pp.data_mean, ctx->st.k, ctx->st.d, x);
    return PCABO_OK;
  }
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  // z travels through the pinned query block (the kernel reads it in place over PCIe: 36 doubles), x comes back the way the
  // acquisition results do - stores to pinned host memory followed by a sequence word the host polls: no copy, no stream
  // synchronisation (40 -> 15 us per BO iteration on the host clock)
  memcpy(ctx->hXq, z, (size_t)ctx->st.k * sizeof(double));
  const unsigned long long seq = ++ctx->seq;
  double* hx = small_at(ctx, small_imap_x(ctx->lay.s));
  launch_inverse_map(s, ctx->hXq, ctx->dComps, ctx->dDataMean, ctx->dPcaMean, ctx->st.k, ctx->st.d, ctx->dXout, nullptr, ZB(),
                     hx, ctx->hm, seq);
  HIPCHK(hipGetLastError());
  const FlagWait w = wait_flags(ctx->hm, 0, 1, seq, deadline_in(20), &s);
  if (w == FLAGS_UNPUBLISHED) {
    HIPCHK(hipGetLastError());
    return set_err(ctx, PCABO_ERR_TIMEOUT, "inverse-map kernel finished without publishing its result%s", "");
  }
  if (w == FLAGS_LATE) return set_err(ctx, PCABO_ERR_TIMEOUT, "device did not publish the inverse map%s", "");
  memcpy(x, hx, (size_t)ctx->st.d * sizeof(double));
  return PCABO_OK;
}

int pcabo_get_gp_state(pcabo_ctx* ctx, double* K_chol, double* Rinv, double* alpha, double* y_mean_std,
                       double* norm_bounds) {
  if (!ctx) return PCABO_ERR_ARG;
  // (a member of a batch that is set aside - pcabo_batch_gp_extend - still holds factors: they are read at the rows it holds)
  if (!ctx->st.holds_factors()) return set_err(ctx, PCABO_ERR_ARG, "pcabo_get_gp_state: call pcabo_gp_condition first%s", "");
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t n = ctx->st.rows_held(), w = n * sizeof(double), pitch = (size_t)ctx->ld * sizeof(double);
  if (K_chol) HIPCHK(hipMemcpy2DAsync(K_chol, w, ctx->dL, pitch, w, n, hipMemcpyDeviceToHost, s));
  if (Rinv) HIPCHK(hipMemcpy2DAsync(Rinv, w, ctx->dR, pitch, w, n, hipMemcpyDeviceToHost, s));
  if (alpha) HOST_OUT(alpha, ctx->dAlpha, n, double);
  HIPCHK(hipStreamSynchronize(s));
  if (y_mean_std) { y_mean_std[0] = ctx->hm->y_mean; y_mean_std[1] = ctx->hm->y_std; }
  if (norm_bounds)
    for (int c = 0; c < ctx->st.k; ++c) { norm_bounds[c] = ctx->hm->norm_lo[c]; norm_bounds[ctx->st.k + c] = ctx->hm->norm_hi[c]; }
  return PCABO_OK;
}

int pcabo_get_gram(pcabo_ctx* ctx, double* K) {
  if (!ctx || !K) return PCABO_ERR_ARG;
  if (!ctx->st.conditioned()) return set_err(ctx, PCABO_ERR_ARG, "pcabo_get_gram: call pcabo_gp_condition first%s", "");
  HIPCHK(hipSetDevice(ctx->device));
  const size_t n = ctx->st.n, w = n * sizeof(double), pitch = (size_t)ctx->ld * sizeof(double);
  // built on demand: the conditioning itself writes only the copy that the factorisation then overwrites
  ctx->st.gram_fetched();
  launch_gram(ctx->stream, ctx->dAT, ctx->dNrm, ctx->st.n, ctx->st.NP, round_up(ctx->st.k, 4), ctx->ld, ctx->st.noise, ctx->st.kernel, ctx->dGram,
              nullptr, nullptr, nullptr);
  HIPCHK(hipMemcpy2DAsync(K, w, ctx->dGram, pitch, w, n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < n; ++i)                  // only the lower tiles are built on the device
    for (size_t j = i + 1; j < n; ++j) K[i * n + j] = K[j * n + i];
  return PCABO_OK;
}

// (pcabo_lbfgsb_minimize, pcabo_lbfgsb_set_vector_kernels, pcabo_sobol_scramble, pcabo_sobol_draw: host_entry.cpp - host code only,
// built by g++ and, for the sanitizer targets of the Makefile, without the HIP runtime)

int pcabo_set_profiling(pcabo_ctx* ctx, int enabled) {
  if (!ctx) return PCABO_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  if (enabled && ctx->pairs.empty()) {
    ctx->pairs.resize(PROF_POOL);
    for (auto& p : ctx->pairs) { HIPCHK(hipEventCreate(&p.a)); HIPCHK(hipEventCreate(&p.b)); p.group = 0; }
  }
  if (!enabled) prof_resolve(ctx);
  if (enabled && !ctx->prof) {
    // calibrate the event-pair overhead on this stream: median reading of 64 back-to-back pairs (nothing in between;
    // subtracted from every pair) - the reading around an EMPTY kernel is reported with PCABO_TRACE_OPT for comparison
    prof_resolve(ctx);
    double med[2] = {0.0, 0.0};
    for (int mode = 0; mode < 2; ++mode) {
      std::vector<float> r;
      for (int i = 0; i < 64; ++i) {
        HIPCHK(hipEventRecord(ctx->pairs[i].a, ctx->stream));
        if (mode == 1) hipLaunchKernelGGL(k_nop, dim3(1), dim3(64), 0, ctx->stream);
        HIPCHK(hipEventRecord(ctx->pairs[i].b, ctx->stream));
      }
      HIPCHK(hipStreamSynchronize(ctx->stream));
      for (int i = 0; i < 64; ++i) { float ms = 0.f; if (hipEventElapsedTime(&ms, ctx->pairs[i].a, ctx->pairs[i].b) == hipSuccess) r.push_back(ms); }
      if (!r.empty()) { std::sort(r.begin(), r.end()); med[mode] = r[r.size() / 2]; }
    }
    ctx->prof_pair_ms = med[0];
    ctx->prof_empty_ms = med[1];
  }
  ctx->prof = enabled != 0;
  return PCABO_OK;
}

int pcabo_get_profile_calibration(pcabo_ctx* ctx, double* pair_ms, double* empty_kernel_ms) {
  if (!ctx) return PCABO_ERR_ARG;
  if (pair_ms) *pair_ms = ctx->prof_pair_ms;
  if (empty_kernel_ms) *empty_kernel_ms = ctx->prof_empty_ms;
  return PCABO_OK;
}

int pcabo_get_profile(pcabo_ctx* ctx, int which, double* ms, int64_t* launches, double* bytes, double* flops) {
  if (!ctx || which < 0 || which >= PROF_GROUPS) return PCABO_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  prof_resolve(ctx);
  if (ms) *ms = ctx->prof_ms[which];
  if (launches) *launches = ctx->prof_launches[which];
  if (bytes) *bytes = ctx->prof_bytes[which];
  if (flops) *flops = ctx->prof_flops[which];
  return PCABO_OK;
}

int pcabo_reset_profile(pcabo_ctx* ctx) {
  if (!ctx) return PCABO_ERR_ARG;
  prof_resolve(ctx);
  for (int i = 0; i < PROF_GROUPS; ++i) { ctx->prof_ms[i] = 0.0; ctx->prof_launches[i] = 0; ctx->prof_bytes[i] = 0.0; ctx->prof_flops[i] = 0.0; }
  return PCABO_OK;
}


// =====================================================================================================================
// Batched contexts (declared in include/pcabo.h): B runs advancing in lock-step.
// =====================================================================================================================
}  // extern "C"

// RestartGroup (one joint L-BFGS-B problem of a run) and GangPool (the batch's worker threads): host_side.h

struct pcabo_batch {
  int device = 0, B = 0, max_n = 0, max_d = 0, max_q = 0;
  hipStream_t stream = nullptr;
  hipEvent_t evPca = nullptr, evBounds = nullptr;
  char *dSlab = nullptr, *hSlab = nullptr;
  size_t zs = 0, hzs = 0;
  std::vector<pcabo_ctx*> ctx;
  std::vector<char> active;              // runs that still take part in pcabo_batch_optimize_acqf (pcabo_batch_set_active)
  BatchState st;                         // where the runs stand together, and the pending _begin halves (model_state.h)
  std::vector<ModelState*> run_st;       // the members' records (ctx[b]->st): written from st by follow() only
  // lock-step fit (pcabo_batch_gp_mll / pcabo_batch_gp_fit): where the last conditioning's inputs lie on the device (run 0); once
  // st.fitted, every batched launch reads 1 / lengthscale from the runs' dHyp blocks
  const double *fitZ = nullptr, *fitY = nullptr, *fitUnb = nullptr;
  int fit_rounds = 0;
  bool prof = false; hipEvent_t pev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // phase marks of the last conditioning
  bool group_acq = true;                 // L-BFGS-B rounds through k_acq_group (pcabo_batch_set_option(PCABO_OPT_GROUP_ACQ, 0): the per-query kernels)
  size_t in_stride_x = 0, in_stride_noise = 0, in_stride_y = 0;   // pcabo_batch_set_input_strides (doubles between two runs' blocks; 0: dense)
  std::vector<int> opt_act;              // the runs of the pcabo_batch_optimize_acqf_begin that has not been ended yet
  int dev_lbfgsb = 0;                    // PCABO_OPT_DEVICE_LBFGSB: 1 device-resident L-BFGS-B, 2 its host-stepped twin
  // debug record of the last optimise call on the device path (pcabo_debug_batch_lbfgsb_*; tests): the twin's branch counters
  // [B][groups][LBB_COUNT], or the eight doubles per group the kernel wrote [B][groups][8]
  std::vector<unsigned> dbg_branches; std::vector<double> dbg_group_out; int dbg_groups = 0;
  char* dPost = nullptr;                             // pcabo_batch_gp_posterior with a covariance: every run's V and cov block,
                                                     // PostSite::post_bytes apart (one allocation, made by the first such call)
  char* dSample = nullptr;                           // pcabo_batch_gp_posterior_sample: every run's SampleBlock, its `bytes` apart
  unsigned *dOptTab = nullptr, *hOptTab = nullptr;   // launch table of the device-resident optimiser (B * 32 entries)
  int G = 0;                             // gangs = worker threads of the L-BFGS-B phase
  std::vector<hipStream_t> gstream;
  GangPool pool;
  std::atomic<unsigned long long> seq{0};
  char err[512] = {0};
};

static int bset_err(pcabo_batch* b, int code, const char* fmt, const char* a = "", int v = 0) {
  if (b) snprintf(b->err, sizeof(b->err), fmt, a, v);
  return code;
}
#define BHIPCHK(call)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) return bset_err(batch, PCABO_ERR_HIP, "HIP error: %s (line %d)", hipGetErrorString(e_), __LINE__); \
  } while (0)

static ZB batch_zb(const pcabo_batch* b) { ZB z; z.B = b->B; z.zs = b->zs; z.hzs = b->hzs; return z; }
// per-run hyperparameter blocks for the batched acquisition launches: only after a lock-step fit (null: the shared scalar)
static const double* batch_hyp(const pcabo_batch* b) { return b->st.fitted ? b->ctx[0]->dHyp : nullptr; }

static void batch_free(pcabo_batch* batch) {
  (void)hipSetDevice(batch->device);
  batch->pool.shutdown();
  if (batch->stream) (void)hipStreamSynchronize(batch->stream);
  for (pcabo_ctx* c : batch->ctx) if (c) { ctx_teardown(c); delete c; }
  for (hipStream_t s : batch->gstream) if (s) (void)hipStreamDestroy(s);
  if (batch->evPca) (void)hipEventDestroy(batch->evPca);
  if (batch->evBounds) (void)hipEventDestroy(batch->evBounds);
  for (hipEvent_t e : batch->pev) if (e) (void)hipEventDestroy(e);
  if (batch->dSlab) (void)hipFree(batch->dSlab);
  if (batch->hSlab) (void)hipHostFree(batch->hSlab);
  if (batch->dPost) (void)hipFree(batch->dPost);
  if (batch->dSample) (void)hipFree(batch->dSample);
  if (batch->dOptTab) (void)hipFree(batch->dOptTab);
  if (batch->hOptTab) (void)hipHostFree(batch->hOptTab);
  if (batch->stream) (void)hipStreamDestroy(batch->stream);
  delete batch;
}

// Rows D-H of all runs on the batch's stream behind whatever the caller has enqueued (enqueue_rows_dh with the batch's strides, k read
// on the device, the batch's phase marks 1..4), the device optimiser's transposed root inverse behind alpha, and the batch's state
// afterwards.  Z / y / unb: run 0's inputs on the device; k >= 0: the reduced dimension of every run, < 0: the wPCA in flight will say.
static int batch_enqueue_condition(pcabo_batch* batch, const double* Z, const double* y, const double* unb, int n, int d, int k,
                                   double lengthscale, double gp_noise, int kernel) {
  pcabo_ctx* c0 = batch->ctx[0];
  hipStream_t s = batch->stream;
  const ZB zb = batch_zb(batch);
  const int NP = round_up(n, PCABO_BS);
  // the tickets of ALL runs are reset when the batch's record or any member's asks for it (a single-context call on a member may
  // have timed out)
  const bool reset = batch->st.tickets_reset_if_needed(acq_slabs(NP), batch->run_st);
  const RowsDH a{Z, y, unb, n, -1, 0, c0->dK, 1.0 / lengthscale, gp_noise, 0.0, kernel, zb,
                 {batch->evBounds, k < 0 ? nullptr : batch->evPca}, reset};
  const int rc = enqueue_rows_dh(c0, s, a, [&](int phase) {
    if (batch->prof) (void)hipEventRecord(batch->pev[phase], s);
    // the device-resident optimiser reads the root inverse transposed as well (the Gram buffer is free: K is only kept on demand)
    if (phase == 4 && batch->dev_lbfgsb) launch_rt_build(s, c0->dR, n, NP, c0->ld, c0->dGram, zb);
    return (int)PCABO_OK;
  });
  if (rc != PCABO_OK) return bset_err(batch, rc, "%s", c0->err);
  BHIPCHK(hipGetLastError());
  batch->st.condition_enqueued(n, d, k, lengthscale, gp_noise, kernel);
  batch->fitZ = Z; batch->fitY = y; batch->fitUnb = unb;
  for (pcabo_ctx* c : batch->ctx) {      // the per-run contexts see the same state (single-context calls keep working)
    if (batch->dev_lbfgsb) c->st.rt_rebuilt();
    c->st.follow(batch->st, c->st.own().with_k(k >= 0 ? k : c->st.k).started(lengthscale, gp_noise));
  }
  return PCABO_OK;
}
static int collect_pending_wpca(pcabo_batch* batch) {
  return batch->st.m.wpca_uncollected ? pcabo_batch_wpca_results(batch, nullptr, nullptr, nullptr, nullptr, nullptr) : PCABO_OK;
}

extern "C" {

int pcabo_batch_create(int device, int B, int max_n, int max_d, int max_q, pcabo_batch** out) {
  if (!out) return PCABO_ERR_ARG;
  *out = nullptr;
  if (B < 1 || B > 4096 || !ctx_sizes_ok(max_n, max_d, max_q)) return PCABO_ERR_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return PCABO_ERR_HIP;
  pcabo_batch* batch = new (std::nothrow) pcabo_batch();
  if (!batch) return PCABO_ERR_HIP;
  *out = batch;                      // handed back even on failure so the caller can read the message (and must destroy it)
  batch->device = device; batch->B = B; batch->max_n = max_n; batch->max_d = max_d; batch->max_q = max_q;
  BHIPCHK(hipSetDevice(device));
  BHIPCHK(hipStreamCreateWithFlags(&batch->stream, hipStreamNonBlocking));
  BHIPCHK(hipEventCreateWithFlags(&batch->evPca, hipEventDisableTiming));
  BHIPCHK(hipEventCreateWithFlags(&batch->evBounds, hipEventDisableTiming));
  const CtxLayout lay = ctx_layout(ctx_shape(max_n, max_d, max_q));      // of every run: run b's regions lie b strides behind run 0's
  batch->zs = lay.dev_bytes; batch->hzs = lay.host_bytes;
  BHIPCHK(hipMalloc((void**)&batch->dSlab, batch->zs * (size_t)B));
  BHIPCHK(hipHostMalloc((void**)&batch->hSlab, batch->hzs * (size_t)B, hipHostMallocDefault));
  memset(batch->hSlab, 0, batch->hzs * (size_t)B);
  BHIPCHK(hipMalloc((void**)&batch->dOptTab, (size_t)B * PCABO_INLAUNCH_MAXQ * sizeof(unsigned)));
  BHIPCHK(hipHostMalloc((void**)&batch->hOptTab, (size_t)B * PCABO_INLAUNCH_MAXQ * sizeof(unsigned), hipHostMallocDefault));
  BHIPCHK(hipMemsetAsync(batch->dSlab, 0, batch->zs * (size_t)B, batch->stream));
  BHIPCHK(hipStreamSynchronize(batch->stream));
  batch->ctx.assign(B, nullptr);
  batch->active.assign(B, 1);
  for (int b = 0; b < B; ++b) {
    pcabo_ctx* c = new (std::nothrow) pcabo_ctx();
    if (!c) return bset_err(batch, PCABO_ERR_HIP, "out of memory%s", "");
    batch->ctx[b] = c;
    batch->run_st.push_back(&c->st);
    int rc = ctx_setup(c, device, lay, batch->dSlab + batch->zs * (size_t)b, batch->hSlab + batch->hzs * (size_t)b, batch->stream);
    c->batch_index = b;
    if (rc != PCABO_OK) return bset_err(batch, rc, "context %s%d of the batch could not be set up", "", b);
  }
  // worker threads of the L-BFGS-B phase: one gang of runs per thread, a HIP stream per gang
  // (hardware_concurrency reports the host, not this process's share of it: a GPU of a shared node comes with ~16 cores,
  // and every worker spins while it waits - 8 by default)
  int T = std::min(8, (int)std::thread::hardware_concurrency() - 2);        // (pcabo_batch_set_workers changes it)
  T = std::max(1, std::min(T, std::min(B, 32)));
  batch->G = T;
  batch->gstream.assign((size_t)T, nullptr);
  for (size_t g = 0; g < batch->gstream.size(); ++g) BHIPCHK(hipStreamCreateWithFlags(&batch->gstream[g], hipStreamNonBlocking));
  batch->pool.start(T);
  for (pcabo_ctx* c : batch->ctx) c->opt_group_acq = batch->group_acq;      // a run's single-context calls match its batch
  batch->seq.store(((unsigned long long)(getpid() & 0xffff) << 44) + (1ull << 43));
  return PCABO_OK;
}

int pcabo_batch_destroy(pcabo_batch* batch) {
  if (!batch) return PCABO_ERR_ARG;
  batch_free(batch);
  return PCABO_OK;
}

// Worker threads (= gangs) of the L-BFGS-B phase.  Every worker spins while its launch is in flight, so the workers of all
// batches of a process should fit the cores the process owns: two batches advancing side by side on two host threads take
// 4 each on a 16-core share.  Not during a call on this batch.  The runs' results do not depend on it.
int pcabo_batch_set_workers(pcabo_batch* batch, int workers) {
  if (!batch || workers < 1) return PCABO_ERR_ARG;
  BHIPCHK(hipSetDevice(batch->device));
  const int T = std::max(1, std::min(workers, std::min(batch->B, 32)));
  if (T == batch->G) return PCABO_OK;
  batch->pool.shutdown();
  BHIPCHK(hipStreamSynchronize(batch->stream));
  for (hipStream_t& s : batch->gstream) if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); s = nullptr; }
  batch->gstream.assign((size_t)T, nullptr);
  for (size_t g = 0; g < batch->gstream.size(); ++g) BHIPCHK(hipStreamCreateWithFlags(&batch->gstream[g], hipStreamNonBlocking));
  batch->G = T;
  batch->pool.start(T);
  return PCABO_OK;
}

// PCABO_OPT_GROUP_ACQ (default 1): the L-BFGS-B rounds of the batch go through the throughput kernel k_acq_group; 0: through
// the per-query kernels a single context uses by default (same formulas, another summation order) - with it a run of the batch
// is bit-identical to the same run in a stand-alone context with default options.  Not during a call on this batch.
int pcabo_batch_set_option(pcabo_batch* batch, int option, int value) {
  if (!batch) return PCABO_ERR_ARG;
  if (option == PCABO_OPT_DEVICE_LBFGSB) {
    if (value < 0 || value > 2) return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_set_option: PCABO_OPT_DEVICE_LBFGSB takes 0, 1 or 2 (%s%d)", "", value);
    // switched on after a conditioning: dGram holds K (or an older RT), not this GP's transposed root inverse - the next
    // launch of the device optimiser rebuilds it (k_rt_build) instead of reading whatever is there
    if (value != 0 && batch->dev_lbfgsb == 0) for (pcabo_ctx* c : batch->ctx) c->st.rt_wanted();
    batch->dev_lbfgsb = value;
    return PCABO_OK;
  }
  if (option != PCABO_OPT_GROUP_ACQ) return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_set_option: unknown option %s%d", "", option);
  batch->group_acq = value != 0;
  for (pcabo_ctx* c : batch->ctx) c->opt_group_acq = batch->group_acq;
  return PCABO_OK;
}

// Device time of the phases of the LAST pcabo_batch_wpca_gp_condition_begin (HIP events on the batch's stream; call after
// the conditioning has been waited for): ms[0] rows A-C (wPCA), ms[1] Normalize + Gram, ms[2] Cholesky, ms[3] root inverse + alpha.
int pcabo_batch_set_profiling(pcabo_batch* batch, int enabled) {
  if (!batch) return PCABO_ERR_ARG;
  BHIPCHK(hipSetDevice(batch->device));
  if (enabled && !batch->pev[0]) for (auto& e : batch->pev) BHIPCHK(hipEventCreate(&e));
  batch->prof = enabled != 0;
  return PCABO_OK;
}
int pcabo_batch_get_profile(pcabo_batch* batch, double* ms) {
  if (!batch || !ms || !batch->prof) return PCABO_ERR_ARG;
  BHIPCHK(hipSetDevice(batch->device));
  BHIPCHK(hipEventSynchronize(batch->pev[4]));
  for (int i = 0; i < 4; ++i) { float t = 0.f; BHIPCHK(hipEventElapsedTime(&t, batch->pev[i], batch->pev[i + 1])); ms[i] = t; }
  return PCABO_OK;
}

// A run whose optimisation cannot go on (botorch would raise there: NaN in the acquisition gradient once the reference's
// unclipped candidates have blown the search box up) is parked by the caller: it stays in the lock-step launches of rows
// A-K (on whatever finite data the caller keeps feeding it) but no longer takes part in pcabo_batch_optimize_acqf.
int pcabo_batch_set_active(pcabo_batch* batch, const int* active) {
  if (!batch || !active) return PCABO_ERR_ARG;
  // between pcabo_batch_gp_extend and the truncate back to n_base a run that did not take part is out of step: nobody changes sides
  if (batch->st.extended())
    for (int b = 0; b < batch->B; ++b)
      if ((active[b] != 0) != (batch->active[b] != 0))
        return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_set_active: points are appended (pcabo_batch_gp_extend); truncate to n_base first%s", "");
  for (int b = 0; b < batch->B; ++b) batch->active[b] = active[b] != 0;
  return PCABO_OK;
}

int pcabo_batch_last_error(pcabo_batch* batch, char* buf, int buflen) {
  if (!batch || !buf || buflen <= 0) return PCABO_ERR_ARG;
  snprintf(buf, buflen, "%s", batch->err);
  return PCABO_OK;
}

pcabo_ctx* pcabo_batch_ctx(pcabo_batch* batch, int b) {
  if (!batch || b < 0 || b >= batch->B) return nullptr;
  return batch->ctx[b];
}

// X, noise and y of pcabo_batch_wpca_gp_condition_begin as they lie in the caller's own arrays: doubles between the blocks of two
// runs (0 = dense, the default).  A driver that keeps X as [B][budget][d] and y as [B][budget] hands the first n rows of every run
// over without building a dense copy per iteration.
int pcabo_batch_set_input_strides(pcabo_batch* batch, size_t x_stride, size_t noise_stride, size_t y_stride) {
  if (!batch) return PCABO_ERR_ARG;
  batch->in_stride_x = x_stride; batch->in_stride_noise = noise_stride; batch->in_stride_y = y_stride;
  return PCABO_OK;
}

int pcabo_batch_wpca_gp_condition_begin(pcabo_batch* batch, const double* X, const int64_t* ranks, const double* noise,
                                        const double* y, int n, int d, int maximize, double var_threshold,
                                        int n_components, double lengthscale, double gp_noise, int kernel) {
  (void)maximize;                    // ranks are given: nothing on the device depends on the direction
  if (!batch) return PCABO_ERR_ARG;
  pcabo_ctx* c0 = batch->ctx[0];
  if (!X || !ranks || !y || n < 2 || n > batch->max_n || d < 1 || d > batch->max_d || !gp_args_ok(c0, n, lengthscale, gp_noise, kernel))
    return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_wpca_gp_condition_begin: bad argument or size beyond the batch's capacity%s", "");
  if (batch->st.m.in_flight()) return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_wpca_gp_condition_begin: a conditioning is in flight%s", "");
  BHIPCHK(hipSetDevice(batch->device));
  hipStream_t s = batch->stream;
  const int B = batch->B;
  const size_t nd = (size_t)n * d;
  // pack [X | noise | ranks | y] of every run into its pinned block; ONE strided copy carries all runs
  const InPack pk = in_pack(n, d, noise != nullptr, true, true);
  const size_t off_noise = pk.noise, off_r = pk.ranks, off_y = pk.y, total = pk.total;
  const size_t sx = batch->in_stride_x ? batch->in_stride_x : nd, sn = batch->in_stride_noise ? batch->in_stride_noise : nd;
  const size_t sy = batch->in_stride_y ? batch->in_stride_y : (size_t)n;
  if (sx < nd || sn < nd || sy < (size_t)n)
    return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_wpca_gp_condition_begin: an input stride is smaller than a run's block%s", "");
  for (int b = 0; b < B; ++b) {
    double* h = batch->ctx[b]->hIn;
    memcpy(h, X + (size_t)b * sx, nd * sizeof(double));
    if (noise) memcpy(h + off_noise, noise + (size_t)b * sn, nd * sizeof(double));
    memcpy(h + off_r, ranks + (size_t)b * n, (size_t)n * 8);
    memcpy(h + off_y, y + (size_t)b * sy, (size_t)n * sizeof(double));
  }
  BHIPCHK(hipMemcpy2DAsync(c0->dIn, batch->zs, c0->hIn, batch->hzs, total * sizeof(double), B, hipMemcpyHostToDevice, s));
  const WpcaInputs in{c0->dIn, noise ? c0->dIn + off_noise : nullptr, c0->dIn + off_y, reinterpret_cast<const long long*>(c0->dIn + off_r)};
  // rows A-C (the ping-pong of ALL runs is the batch's: they advance together)
  const int rc = enqueue_rows_ac(c0, s, batch->st.m, in, n, d, var_threshold, n_components, batch_zb(batch), batch->evPca, [&](int behind) {
    if (!behind && batch->prof) (void)hipEventRecord(batch->pev[0], s);
  });
  if (rc != PCABO_OK) return bset_err(batch, rc, "%s", c0->err);
  // rows D-H, queued behind the projection (k is read on the device)
  return batch_enqueue_condition(batch, c0->dZ, in.y, nullptr, n, d, -1, lengthscale, gp_noise, kernel);
}

// Rows D-H for every run WITHOUT the weighted PCA: the GPs live on the given points (pcabo_gp_condition_begin for B runs; the
// reference's Vanilla_BO, Vanilla_BO.py:166-196, conditions on the raw d-dimensional points with Normalize switched off - the
// caller passes identity bounds).  Z[B][n*k] and y[B][n] (strides: pcabo_batch_set_input_strides), norm_bounds[2*k] for all runs
// (lo[k], hi[k]) or NULL (bounds from the data as for PCA_BO).  Finish with pcabo_batch_gp_condition_end_eval.
int pcabo_batch_gp_condition_begin(pcabo_batch* batch, const double* Z, const double* y, int n, int k, const double* norm_bounds,
                                   double lengthscale, double gp_noise, int kernel) {
  if (!batch) return PCABO_ERR_ARG;
  pcabo_ctx* c0 = batch->ctx[0];
  if (!Z || !y || n < 2 || n > batch->max_n || k < 1 || k > batch->max_d || !gp_args_ok(c0, n, lengthscale, gp_noise, kernel))
    return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_gp_condition_begin: bad argument or size beyond the batch's capacity%s", "");
  if (batch->st.m.in_flight()) return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_gp_condition_begin: a conditioning is in flight%s", "");
  BHIPCHK(hipSetDevice(batch->device));
  hipStream_t s = batch->stream;
  const int B = batch->B;
  const size_t nk = (size_t)n * k, off_y = in_pack(n, k, false, false, true).y, total = in_pack(n, k, false, false, true).total;
  const size_t sx = batch->in_stride_x ? batch->in_stride_x : nk, sy = batch->in_stride_y ? batch->in_stride_y : (size_t)n;
  if (sx < nk || sy < (size_t)n)
    return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_gp_condition_begin: an input stride is smaller than a run's block%s", "");
  for (int b = 0; b < B; ++b) {
    pcabo_ctx* c = batch->ctx[b];
    memcpy(c->hIn, Z + (size_t)b * sx, nk * sizeof(double));
    memcpy(c->hIn + off_y, y + (size_t)b * sy, (size_t)n * sizeof(double));
    c->hm->k = k;
    if (norm_bounds) memcpy(small_at(c, small_norm_bounds(c->lay.s)), norm_bounds, (size_t)2 * k * sizeof(double));
  }
  BHIPCHK(hipMemcpy2DAsync(c0->dIn, batch->zs, c0->hIn, batch->hzs, total * sizeof(double), B, hipMemcpyHostToDevice, s));
  BHIPCHK(hipMemcpy2DAsync(c0->dK, batch->zs, &c0->hm->k, batch->hzs, sizeof(int), B, hipMemcpyHostToDevice, s));
  if (norm_bounds)
    BHIPCHK(hipMemcpy2DAsync(c0->dUserNB, batch->zs, small_at(c0, small_norm_bounds(c0->lay.s)), batch->hzs, (size_t)2 * k * sizeof(double), B,
                             hipMemcpyHostToDevice, s));
  if (batch->prof) (void)hipEventRecord(batch->pev[0], s);
  return batch_enqueue_condition(batch, c0->dIn, c0->dIn + off_y, norm_bounds ? c0->dUserNB : nullptr, n, k, k, lengthscale, gp_noise, kernel);
}

int pcabo_batch_wpca_results(pcabo_batch* batch, double* data_mean, double* pca_mean, double* comps, double* evr, int* k) {
  if (!batch) return PCABO_ERR_ARG;
  if (!batch->st.anything_enqueued()) return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_wpca_results: nothing enqueued%s", "");
  BHIPCHK(hipSetDevice(batch->device));
  BHIPCHK(wait_event(batch->evPca));
  BHIPCHK(hipGetLastError());
  const int n = batch->st.m.n, d = batch->st.m.d, rcount = n < d ? n : d;
  batch->st.wpca_collected();
  for (int b = 0; b < batch->B; ++b) {
    pcabo_ctx* c = batch->ctx[b];
    wpca_hand_out(c, d, rcount, data_mean ? data_mean + (size_t)b * d : nullptr, pca_mean ? pca_mean + (size_t)b * d : nullptr,
                  comps ? comps + (size_t)b * d * d : nullptr, evr ? evr + (size_t)b * d : nullptr);
    c->st.follow(batch->st, c->st.own().with_k(c->hm->k));
    if (k) k[b] = c->st.k;
  }
  return PCABO_OK;
}

int pcabo_batch_acq_bounds(pcabo_batch* batch, double* bounds) {
  if (!batch || !bounds) return PCABO_ERR_ARG;
  if (const int rc = collect_pending_wpca(batch)) return rc;
  if (batch->st.m.in_flight()) {
    BHIPCHK(hipSetDevice(batch->device));
    BHIPCHK(wait_event(batch->evBounds));
  } else if (!batch->st.m.conditioned()) {
    return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_acq_bounds: no conditioning enqueued%s", "");
  }
  for (int b = 0; b < batch->B; ++b) {
    const pcabo_ctx* c = batch->ctx[b];
    double* o = bounds + (size_t)b * 2 * batch->max_d;
    for (int j = 0; j < c->st.k; ++j) { o[j] = c->hm->acq_lo[j]; o[c->st.k + j] = c->hm->acq_hi[j]; }
  }
  return PCABO_OK;
}

static int batch_max_k(const pcabo_batch* batch) {
  int km = 1;
  for (const pcabo_ctx* c : batch->ctx) km = std::max(km, c->st.k);
  return km;
}

// the conditioned model of all runs as the batched launchers take it: run 0's operands (the others lie zs bytes apart each), the
// batch's n / NP, the largest k of the runs
static GpModel gp_model(const pcabo_batch* batch, int kmax) {
  GpModel m = gp_model(batch->ctx[0]);
  m.n = batch->st.m.n; m.k = kmax; m.NP = batch->st.m.NP;
  return m;
}
// the acquisition constants of a batched launch (best_f travels per run: batch_put_best_f)
static AcqParams batch_params(const pcabo_batch* batch, int maximize, int acq, int want_grad) {
  AcqParams p = make_params(batch->ctx[0], 0.0, maximize, acq, want_grad);
  p.inv_ls = 1.0 / batch->st.m.lengthscale; p.kernel = batch->st.m.kernel;
  return p;
}

static AcqBatch batch_ab(const pcabo_batch* batch, int table, int xq_host) {
  AcqBatch ab;
  ab.zs = batch->zs; ab.hzs = batch->hzs; ab.k_dev = batch->ctx[0]->dK; ab.bestf = batch->ctx[0]->dBestF;
  ab.table = table; ab.xq_host = xq_host; ab.hyp = batch_hyp(batch);
  return ab;
}

// acq_arg_error for a batch call: the scalars of the active runs only (a parked run's slot is never read by a kernel that counts)
static const char* batch_acq_arg_error(const pcabo_batch* batch, int acq, const double* best_f) {
  if (const char* why = acq_arg_error(acq, 0.0)) return why;
  for (int b = 0; b < batch->B; ++b)
    if (batch->active[b])
      if (const char* why = acq_arg_error(acq, best_f[b])) return why;
  return nullptr;
}

// best_f of every run (PCABO_ACQ_UCB: its kappa) -> its device word (rounded per run like the single-context calls do)
static int batch_put_best_f(pcabo_batch* batch, const double* best_f) {
  pcabo_ctx* c0 = batch->ctx[0];
  for (int b = 0; b < batch->B; ++b) {
    pcabo_ctx* c = batch->ctx[b];
    c->hBestF[0] = c->bestf_f32 ? (double)(float)best_f[b] : best_f[b];
  }
  BHIPCHK(hipMemcpy2DAsync(c0->dBestF, batch->zs, c0->hBestF, batch->hzs, sizeof(double), batch->B, hipMemcpyHostToDevice, batch->stream));
  return PCABO_OK;
}

}  // extern "C"

// ---- lock-step GP hyperparameter fit of a batch (DESIGN.md "GP hyperparameter fit", the batched form) -------------------
// One round = ONE launch sequence for all B runs (blockIdx.z = run): every run is conditioned at its own theta, read by k_zstats,
// k_znorm and k_gram from the runs' dHyp blocks, then k_mll_grad + k_mll_finish, one strided copy of the runs' results and one wait.
// All runs of a round have one form of the model: the shared lengthscale (m = 1 rho, 3 variables each, 6 results) or, ard, one
// lengthscale per input (run b: m = k_b, 5 + KP_b results; the copy brings 5 + KP_max doubles per run).  In the ARD form a run's
// lengthscales softplus(rho_c) travel in its dArdLs (one strided copy per round) and k_zstats folds them into its Normalize ranges
// where word PCABO_HYP_ARD_FOLD of its block says so; its 1 / lengthscale is 1.
// hyp_theta[b]: the theta run b is conditioned at, or NULL for a run that rests at the batch's shared model (parked runs): the
// shared lengthscale, no fold.
// A run whose Cholesky failed in the round is redone alone on its own context (mll_attempts from the first jitter on), as
// batch_score_collect does; st[b] is PCABO_OK, PCABO_ERR_NOT_PD or a HIP error for every run with a theta, untouched otherwise.
static int batch_fit_m(const pcabo_batch* batch, bool ard, int b) { return ard ? batch->ctx[b]->st.k : 1; }
static int batch_mll_round(pcabo_batch* batch, bool ard, const std::vector<const double*>& hyp_theta, int* st) {
  const int B = batch->B, n = batch->st.m.n, NP = batch->st.m.NP;
  pcabo_ctx* c0 = batch->ctx[0];
  hipStream_t s = batch->stream;
  const int kmax = batch_max_k(batch), Mmax = ard ? round_up(kmax, 4) : 1;
  for (int b = 0; b < B; ++b) {
    pcabo_ctx* c = batch->ctx[b];
    const double* th = hyp_theta[b];
    // the very doubles the single-context path passes by value: 1.0 / softplus(rho) (ard: 1.0 / 1.0), the noise, the mean constant
    const bool fold = ard && th;
    const double ls = !th ? batch->st.m.lengthscale : (ard ? 1.0 : softplus_host(th[2]));
    c->hHyp[PCABO_HYP_INV_LS] = 1.0 / ls;
    c->hHyp[PCABO_HYP_NOISE] = th ? th[0] : batch->st.m.noise;
    c->hHyp[PCABO_HYP_MEAN_C] = th ? th[1] : 0.0;
    c->hHyp[PCABO_HYP_ARD_FOLD] = fold ? 1.0 : 0.0;
    if (fold)                            // the very doubles mll_launch writes for a single context
      for (int j = 0; j < c->st.k; ++j) c->hArdLs[j] = softplus_host(th[2 + j]);
    c->st.follow(batch->st, c->st.own().started(ls, c->hHyp[PCABO_HYP_NOISE]));   // single-context calls on a member see its model
  }
  BHIPCHK(hipMemcpy2DAsync(c0->dHyp, batch->zs, c0->hHyp, batch->hzs, PCABO_HYP_WORDS * sizeof(double), B, hipMemcpyHostToDevice, s));
  if (ard) BHIPCHK(hipMemcpy2DAsync(c0->dArdLs, batch->zs, c0->hArdLs, batch->hzs, (size_t)kmax * sizeof(double), B, hipMemcpyHostToDevice, s));
  ZB zb = batch_zb(batch);
  zb.hyp = c0->dHyp;
  const RowsDH a{batch->fitZ, batch->fitY, batch->fitUnb, n, -1, 0, c0->dK, 0.0, 0.0, 0.0, batch->st.m.kernel, zb, {nullptr, nullptr}, false,
                 ard ? c0->dArdLs : nullptr};
  const int rc = enqueue_rows_dh(c0, s, a, [&](int phase) -> int {
    if (phase != 4) return PCABO_OK;     // behind alpha: the likelihood kernels and the strided copy of the runs' results
    pcabo_ctx* ctx = c0;
    double* out = c0->dMll + mll_result(NP, Mmax).start;      // one place for all runs, behind the widest run's tile partials
    launch_mll_grad(s, ard, c0->dR, c0->dAT, c0->dNrm, c0->dAlpha, c0->dL, c0->dYs, n, NP, 0, c0->ld, c0->dMll, out, c0->dK, zb);
    HIPCHK(hipMemcpy2DAsync(c0->hMll, batch->hzs, out, batch->zs, mll_result(NP, Mmax).count * sizeof(double), B, hipMemcpyDeviceToHost, s));
    return PCABO_OK;
  });
  if (rc != PCABO_OK) return bset_err(batch, rc, "%s", c0->err);
  BHIPCHK(wait_stream(s));
  BHIPCHK(hipGetLastError());
  ++batch->fit_rounds;
  for (int b = 0; b < B; ++b) {
    pcabo_ctx* c = batch->ctx[b];
    if (c->hm->chol_info == 0) { c->st.follow(batch->st, c->st.own().ended(true)); if (hyp_theta[b]) st[b] = PCABO_OK; continue; }
    if (!hyp_theta[b]) continue;
    st[b] = mll_attempts(c, 1, ard);     // rare: jitter 1e-8, 1e-7, 1e-6 for this run alone (its own record is told how it ended)
  }
  return PCABO_OK;
}

// what both entry points need before the first round; *act = the runs that take part.  ld_theta: doubles between two runs' thetas
// (the ARD form: at least 2 + the largest k of the runs, known once the wPCA results are in)
static int batch_fit_prepare(pcabo_batch* batch, const char* who, bool ard, int ld_theta, std::vector<char>* act, int* status) {
  if (batch->st.m.kernel != PCABO_KERNEL_MATERN52 && (batch->st.m.in_flight() || batch->st.m.conditioned()))
    return bset_err(batch, PCABO_ERR_ARG, "%s: the fit is restated for the Matern-5/2 kernel only", who);
  if (!batch->st.scorable() || !batch->fitZ)
    return bset_err(batch, PCABO_ERR_ARG, "%s: call pcabo_batch_wpca_gp_condition_begin or pcabo_batch_gp_condition_begin first", who);
  if (batch->st.begin_pending())
    return bset_err(batch, PCABO_ERR_ARG, "%s: a _begin call of this batch has not been ended", who);
  BHIPCHK(hipSetDevice(batch->device));
  if (const int rc = collect_pending_wpca(batch)) return rc;
  if (ard && ld_theta < 2 + batch_max_k(batch))
    return bset_err(batch, PCABO_ERR_ARG, "%s: ld_theta is smaller than 2 + the largest reduced dimension of the runs (%d)", who, 2 + batch_max_k(batch));
  act->assign((size_t)batch->B, 0);
  for (int b = 0; b < batch->B; ++b) {
    (*act)[b] = batch->active[b] ? 1 : 0;
    if (status) status[b] = batch->active[b] ? PCABO_OK : PCABO_ERR_ARG;
  }
  // behind the last refusal (a refused call changes nothing): points appended by pcabo_batch_gp_extend are forgotten, the fit starts
  // over from the n_base it was given; the first round's follow() tells the members
  if (batch->st.extended()) {
    batch->st.extension_forgotten();
    if (batch->st.tickets_reset_if_needed(acq_slabs(batch->st.m.NP), batch->run_st))
      BHIPCHK(hipMemset2DAsync(batch->ctx[0]->dCounters, batch->zs, 0, ticket_bytes(batch->ctx[0]), batch->B, batch->stream));
  }
  return PCABO_OK;
}

// the batch after its last round: conditioned (and waited for), every run at its own model
static void batch_fit_done(pcabo_batch* batch) {
  batch->st.fit_finished();
  // the device-resident optimiser reads the transposed root inverse of the FINAL factorisation (stream order: before its launch)
  if (batch->dev_lbfgsb) {
    pcabo_ctx* c0 = batch->ctx[0];
    launch_rt_build(batch->stream, c0->dR, batch->st.m.n, batch->st.m.NP, c0->ld, c0->dGram, batch_zb(batch));
    for (pcabo_ctx* c : batch->ctx) c->st.rt_rebuilt();
  }
}

// pcabo_batch_gp_mll / pcabo_batch_gp_mll_ard: row b of theta and grad starts ld doubles behind row b - 1 (2 + m_b of them used)
static int batch_gp_mll_call(pcabo_batch* batch, const char* who, bool ard, const double* theta, int ld, double* loss, double* grad,
                             int* status) {
  if (!batch) return PCABO_ERR_ARG;
  if (!theta || !loss) return bset_err(batch, PCABO_ERR_ARG, "%s: theta and loss are required", who);
  std::vector<char> act;
  int rc = batch_fit_prepare(batch, who, ard, ld, &act, status);
  if (rc != PCABO_OK) return rc;
  const int B = batch->B;
  std::vector<const double*> th((size_t)B, nullptr);
  std::vector<int> st((size_t)B, PCABO_ERR_ARG);
  for (int b = 0; b < B; ++b) {
    if (!act[b]) continue;
    const double* t = theta + (size_t)ld * b;
    if (mll_theta_ok(t, batch_fit_m(batch, ard, b))) th[b] = t;
    else theta_domain_err(batch->ctx[b], who, ard);
  }
  batch->fit_rounds = 0;
  rc = batch_mll_round(batch, ard, th, st.data());
  if (rc != PCABO_OK) return rc;
  batch_fit_done(batch);
  int worst = PCABO_OK;
  for (int b = 0; b < B; ++b) {
    if (st[b] == PCABO_OK)
      mll_assemble(batch->ctx[b]->hMll, batch->st.m.n, batch_fit_m(batch, ard, b), theta + (size_t)ld * b, loss + b,
                   grad ? grad + (size_t)ld * b : nullptr);
    else if (act[b]) worst = st[b];
    if (status) status[b] = st[b];
  }
  if (worst != PCABO_OK && !status) return bset_err(batch, worst, "%s: a run of the batch failed (status array not given)", who);
  return PCABO_OK;
}

// pcabo_batch_gp_fit / pcabo_batch_gp_fit_ard
static int batch_gp_fit_call(pcabo_batch* batch, const char* who, bool ard, double* theta_inout, int ld, double* loss, int* info,
                             int* status) {
  if (!batch) return PCABO_ERR_ARG;
  if (!theta_inout) return bset_err(batch, PCABO_ERR_ARG, "%s: theta_inout is required", who);
  std::vector<char> act;
  int rc = batch_fit_prepare(batch, who, ard, ld, &act, status);
  if (rc != PCABO_OK) return rc;
  const int B = batch->B;
  std::vector<FitRun> runs((size_t)B);                   // (a parked run stays OUT: it rides along at the shared model)
  for (int b = 0; b < B; ++b) {
    runs[b].bind(batch->ctx[b]->hMll);
    if (act[b]) runs[b].init(theta_inout + (size_t)ld * b, batch_fit_m(batch, ard, b), ard);
  }
  batch->fit_rounds = 0;
  const auto round = [&](const std::vector<const double*>& th, int* st) { return batch_mll_round(batch, ard, th, st); };
  rc = fit_rounds(runs, batch->st.m.n, round);
  // (no run wanted an evaluation: one round all the same, the batch is left conditioned at the shared model)
  if (rc == PCABO_OK && batch->fit_rounds == 0) rc = round(std::vector<const double*>((size_t)B, nullptr), nullptr);
  if (rc != PCABO_OK) return rc;
  batch_fit_done(batch);
  int worst = PCABO_OK;
  for (int b = 0; b < B; ++b) {
    const FitRun& r = runs[b];
    if (status) status[b] = r.status;
    if (!act[b]) continue;
    if (r.status == PCABO_ERR_ARG) theta_domain_err(batch->ctx[b], who, ard);
    if (r.status != PCABO_OK) { worst = r.status; batch->ctx[b]->st.follow(batch->st, batch->ctx[b]->st.own().ended(false)); continue; }
    memcpy(theta_inout + (size_t)ld * b, r.xr, (size_t)r.nvar * sizeof(double));
    if (loss) loss[b] = r.fr;
    if (info) r.report(info + 4 * b);
  }
  if (worst != PCABO_OK && !status) return bset_err(batch, worst, "%s: a run of the batch failed (status array not given)", who);
  return PCABO_OK;
}

extern "C" {

int pcabo_batch_gp_mll(pcabo_batch* batch, const double* theta, double* loss, double* grad, int* status) {
  return batch_gp_mll_call(batch, "pcabo_batch_gp_mll", false, theta, 3, loss, grad, status);
}
int pcabo_batch_gp_fit(pcabo_batch* batch, double* theta_inout, double* loss, int* info, int* status) {
  return batch_gp_fit_call(batch, "pcabo_batch_gp_fit", false, theta_inout, 3, loss, info, status);
}
// The ARD form (DESIGN.md "ARD lengthscales"): row b of theta = (s2, c, rho_1 .. rho_{k_b}) in ld_theta >= 2 + max_b k_b doubles;
// what lies beyond 2 + k_b in a row is neither read nor written (grad has the same layout).
int pcabo_batch_gp_mll_ard(pcabo_batch* batch, const double* theta, int ld_theta, double* loss, double* grad, int* status) {
  return batch_gp_mll_call(batch, "pcabo_batch_gp_mll_ard", true, theta, ld_theta, loss, grad, status);
}
int pcabo_batch_gp_fit_ard(pcabo_batch* batch, double* theta_inout, int ld_theta, double* loss, int* info, int* status) {
  return batch_gp_fit_call(batch, "pcabo_batch_gp_fit_ard", true, theta_inout, ld_theta, loss, info, status);
}

// launch sequences (rounds) the last pcabo_batch_gp_fit / pcabo_batch_gp_mll took: with the runs' evaluation counts it gives
// the share of run-evaluations spent on runs that had already finished
int pcabo_batch_gp_fit_rounds(pcabo_batch* batch) { return batch ? batch->fit_rounds : PCABO_ERR_ARG; }

}  // extern "C"

extern "C" {

// The scoring of the raw samples in two halves: _begin packs the points, enqueues copy - scoring launch - copy back and
// returns; _end waits for the stream and finishes (jitter retries of single runs included).  pcabo_batch_busy tells a caller
// that drives several batches from one thread when _end (or any other waiting call) would return at once.
int pcabo_batch_busy(pcabo_batch* batch) {
  if (!batch) return PCABO_ERR_ARG;
  if (hipSetDevice(batch->device) != hipSuccess) return PCABO_ERR_HIP;
  const hipError_t e = hipStreamQuery(batch->stream);
  return e == hipErrorNotReady ? 1 : (e == hipSuccess ? 0 : PCABO_ERR_HIP);
}

// What both halves of the scoring check (_end takes the call's arguments again: it needs them for a run it has to redo alone).
// out_ok: the caller's val is there - asked before anything is written, also when only the second half will use it.
static int batch_score_args(pcabo_batch* batch, const double* Xq, int q, const double* best_f, int acq, bool out_ok) {
  if (!Xq || !best_f || !out_ok || q < 1 || q > batch->max_q)
    return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_gp_condition_end_eval: bad argument%s", "");
  if (const char* why = batch_acq_arg_error(batch, acq, best_f)) return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_gp_condition_end_eval: %s", why);
  // (after pcabo_batch_gp_fit the conditioning has been waited for already: the fitted state is scored by the same launches)
  if (!batch->st.scorable()) return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_gp_condition_end_eval: no conditioning in flight%s", "");
  return PCABO_OK;
}

// The launches of a scoring of all runs' queries on the batch's model as it stands: queries packed and copied, the values' launch
// (the GEMM route from q = 64, the per-query kernels below), the values on their way back to every run's hVal.
static int batch_score_launch(pcabo_batch* batch, const double* Xq, int q, const double* best_f, int maximize, int acq) {
  if (const int rc = collect_pending_wpca(batch)) return rc;
  BHIPCHK(hipSetDevice(batch->device));
  hipStream_t s = batch->stream;
  const int B = batch->B, kmax = batch_max_k(batch);
  pcabo_ctx* c0 = batch->ctx[0];
  for (int b = 0; b < B; ++b)
    memcpy(batch->ctx[b]->hXq, Xq + (size_t)b * q * batch->max_d, (size_t)q * batch->ctx[b]->st.k * sizeof(double));
  BHIPCHK(hipMemcpy2DAsync(c0->dXq, batch->zs, c0->hXq, batch->hzs, (size_t)q * kmax * sizeof(double), B, hipMemcpyHostToDevice, s));
  if (const int rc = batch_put_best_f(batch, best_f)) return rc;
  const AcqParams p = batch_params(batch, maximize, acq, 0);
  if (score_gemm_possible(q))
    launch_score(s, c0->dXq, q, gp_model(batch, kmax), p, c0->dKS, c0->dPartial, c0->dVal, batch_ab(batch, 0, 0), B);
  else
    launch_acq(s, nullptr, c0->dXq, q, gp_model(batch, kmax), p, c0->dPartial, c0->dCounters, c0->dVal, c0->dGrad, nullptr, nullptr,
               nullptr, 0, nullptr, nullptr, batch_ab(batch, 0, 0), B, 0);
  BHIPCHK(hipMemcpy2DAsync(c0->hVal, batch->hzs, c0->dVal, batch->zs, (size_t)q * sizeof(double), B, hipMemcpyDeviceToHost, s));
  BHIPCHK(hipGetLastError());
  return PCABO_OK;
}

static int batch_score_enqueue(pcabo_batch* batch, const double* Xq, int q, const double* best_f, int maximize, int acq, bool out_ok = true) {
  if (!batch) return PCABO_ERR_ARG;
  if (const int rc = batch_score_args(batch, Xq, q, best_f, acq, out_ok)) return rc;
  if (batch->st.score_enqueued) return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_gp_condition_end_eval: a scoring is already enqueued%s", "");
  if (batch->st.value_score_enqueued)
    return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_gp_condition_end_eval: a pcabo_batch_acq_score_begin has not been ended%s", "");
  if (const int rc = batch_score_launch(batch, Xq, q, best_f, maximize, acq)) return rc;
  batch->st.scoring_begun();
  return PCABO_OK;
}

static int batch_score_collect(pcabo_batch* batch, const double* Xq, int q, const double* best_f, int maximize, int acq, double* val,
                               int* status) {
  if (!batch) return PCABO_ERR_ARG;
  if (!batch->st.score_enqueued) return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_gp_condition_end_eval_end: no _begin before it%s", "");
  if (const int rc = batch_score_args(batch, Xq, q, best_f, acq, val != nullptr)) return rc;
  BHIPCHK(hipSetDevice(batch->device));
  BHIPCHK(wait_stream(batch->stream));
  BHIPCHK(hipGetLastError());
  batch->st.scoring_ended();
  int worst = PCABO_OK;
  for (int b = 0; b < batch->B; ++b) {
    pcabo_ctx* c = batch->ctx[b];
    int st = PCABO_OK;
    if (c->st.own().is_aside()) {
      // a scoring of an extended, fitted batch: a run set aside (pcabo_batch_gp_extend) holds fewer points than were scored - it is
      // skipped like a run without a GP, its block of val left alone, and it stays aside
      c->st.follow(batch->st, c->st.own().ended(false));
      if (status) status[b] = PCABO_ERR_ARG;
      continue;
    }
    if (c->hm->chol_info != 0) {
      // rare: this run's K needed jitter (psd_safe_cholesky: 1e-8, 1e-7, 1e-6) - redo it alone (its own record is told how that
      // ended), then score again
      st = factor_attempts(c, 1);
      if (st == PCABO_OK) {
        if (batch->dev_lbfgsb) { launch_rt_build(c->stream, c->dR, c->st.n, c->st.NP, c->ld, c->dGram); c->st.rt_rebuilt(); }
        st = pcabo_acq_eval(c, Xq + (size_t)b * q * batch->max_d, q, best_f[b], maximize, acq, c->hVal, nullptr);
      }
    }
    c->st.follow(batch->st, c->st.own().ended(st == PCABO_OK));
    if (st == PCABO_OK) memcpy(val + (size_t)b * q, c->hVal, (size_t)q * sizeof(double));
    if (status) status[b] = st;
    if (st != PCABO_OK) worst = st;
  }
  if (worst != PCABO_OK && !status) return bset_err(batch, worst, "a run of the batch failed in the conditioning (status array not given)%s", "");
  return PCABO_OK;
}

// pcabo_batch_acq_score: the same launches on a model that is there already (BatchState::value_scorable) - values only, nothing of
// the model's phase changes, no run is redone alone.  A run that is parked, set aside or without a GP is computed with the others
// and not handed out.
static int batch_value_score_args(pcabo_batch* batch, const double* Xq, int q, const double* best_f, int acq, bool out_ok) {
  if (!Xq || !best_f || !out_ok || q < 1 || q > batch->max_q) return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_acq_score: bad argument%s", "");
  if (const char* why = batch_acq_arg_error(batch, acq, best_f)) return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_acq_score: %s", why);
  return PCABO_OK;
}
static int batch_value_score_enqueue(pcabo_batch* batch, const double* Xq, int q, const double* best_f, int maximize, int acq, bool out_ok = true) {
  if (!batch) return PCABO_ERR_ARG;
  if (const int rc = batch_value_score_args(batch, Xq, q, best_f, acq, out_ok)) return rc;
  if (!batch->st.value_scorable())
    return bset_err(batch, PCABO_ERR_ARG, batch->st.gp_ready() == GP_IN_FLIGHT
                        ? "pcabo_batch_acq_score: a conditioning or a _begin call of this batch has not been ended%s"
                        : "pcabo_batch_acq_score: no conditioned GP%s", "");
  if (const int rc = batch_score_launch(batch, Xq, q, best_f, maximize, acq)) return rc;
  batch->st.value_scoring_begun();
  return PCABO_OK;
}
static int batch_value_score_collect(pcabo_batch* batch, int q, double* val, int* status) {
  if (!batch) return PCABO_ERR_ARG;
  if (!batch->st.value_score_enqueued) return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_acq_score_end: no _begin before it%s", "");
  if (!val || q < 1 || q > batch->max_q) return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_acq_score_end: bad argument%s", "");
  BHIPCHK(hipSetDevice(batch->device));
  BHIPCHK(wait_stream(batch->stream));
  BHIPCHK(hipGetLastError());
  batch->st.value_scoring_ended();
  for (int b = 0; b < batch->B; ++b) {
    pcabo_ctx* c = batch->ctx[b];
    const bool live = batch->active[b] && c->st.conditioned();
    if (live) memcpy(val + (size_t)b * q, c->hVal, (size_t)q * sizeof(double));
    if (status) status[b] = live ? PCABO_OK : PCABO_ERR_ARG;
  }
  return PCABO_OK;
}

int pcabo_batch_acq_score(pcabo_batch* batch, const double* Xq, int q, const double* best_f, int maximize, int acq, double* val,
                          int* status) {
  const int rc = batch_value_score_enqueue(batch, Xq, q, best_f, maximize, acq, val != nullptr);
  return rc != PCABO_OK ? rc : batch_value_score_collect(batch, q, val, status);
}
int pcabo_batch_acq_score_begin(pcabo_batch* batch, const double* Xq, int q, const double* best_f, int maximize, int acq) {
  return batch_value_score_enqueue(batch, Xq, q, best_f, maximize, acq);
}
int pcabo_batch_acq_score_end(pcabo_batch* batch, int q, double* val, int* status) {
  return batch_value_score_collect(batch, q, val, status);
}

int pcabo_batch_gp_condition_end_eval(pcabo_batch* batch, const double* Xq, int q, const double* best_f, int maximize,
                                      int acq, double* val, int* status) {
  const int rc = batch_score_enqueue(batch, Xq, q, best_f, maximize, acq, val != nullptr);
  return rc != PCABO_OK ? rc : batch_score_collect(batch, Xq, q, best_f, maximize, acq, val, status);
}
int pcabo_batch_gp_condition_end_eval_begin(pcabo_batch* batch, const double* Xq, int q, const double* best_f, int maximize, int acq) {
  return batch_score_enqueue(batch, Xq, q, best_f, maximize, acq);
}
int pcabo_batch_gp_condition_end_eval_end(pcabo_batch* batch, const double* Xq, int q, const double* best_f, int maximize,
                                          int acq, double* val, int* status) {
  return batch_score_collect(batch, Xq, q, best_f, maximize, acq, val, status);
}

// ---- posterior queries and samples, of a context and of the runs of a batch (DESIGN.md "GP posterior queries" / "samples") -----
// Query: the scoring launches up to the scalar chain, then mean and variance per query and, on request, the joint covariance
// (kernels_post.hip).  The queries go straight from the caller's array to dXq: of the state only dXq, dKS and dPartial are written,
// which every evaluation writes before it reads.  No sequence number is taken, no ticket touched, the second stream not used.
// Samples: the query with its covariance, then cov + j s_y^2 I factored in a block of its own and the triangular product with the
// caller's base samples.  The factorisation is the GP's (launch_cholesky) on the sample block's own info word and scratch tiles:
// dInfo, dDiag and the host mirror's chol_info belong to the GP's factorisation and are not touched.
// A batch is one launch sequence (blockIdx.z = run), every run at its own k and - after a lock-step fit - its own lengthscale and
// noise; parked runs and runs without a GP are computed with the others and not handed out.  A context is the same with one run.
static const char* post_arg_error(const double* Xq, int q, int max_q, int flags, bool any_out, int known = PCABO_POST_OBS_NOISE) {
  if (!Xq) return "Xq is required";
  if (q < 1 || q > max_q) return "q must lie in 1 .. max_q";
  if (!any_out) return "mean, var and cov are all NULL";
  if (flags & ~known) return "unknown flag bits";
  return nullptr;
}
// ... and what a sampling call adds to them
static const char* sample_arg_error(const double* Xq, int q, int max_q, int flags, const double* base, int S, const double* samples) {
  if (const char* why = post_arg_error(Xq, q, max_q, flags, true, PCABO_POST_OBS_NOISE | PCABO_POST_CENTRED)) return why;
  if (!base || !samples) return "base and samples are required";
  if (S < 1 || S > PCABO_POST_MAX_SAMPLES) return "S must lie in 1 .. PCABO_POST_MAX_SAMPLES";
  return nullptr;
}

// One run's sample block: factor | two scratch tiles | base | samples | info word.  launch_cholesky applies ONE stride to the matrix,
// the info word and the scratch, so in a batch the runs' blocks lie `bytes` apart and that stride serves all of them.
struct SampleBlock {
  size_t factor, diag, base, out, info, bytes;        // byte offsets inside the block; bytes: the block, a multiple of 256
  explicit SampleBlock(int max_q) {
    const size_t QP = (size_t)round_up(max_q, PCABO_BS), cap = (size_t)PCABO_POST_MAX_SAMPLES * max_q;
    factor = 0;
    diag = factor + QP * QP * sizeof(double);
    base = diag + (size_t)2 * PCABO_BS * PCABO_BS * sizeof(double);
    out = base + cap * sizeof(double);
    info = out + cap * sizeof(double);
    bytes = (info + sizeof(int) + 255) & ~(size_t)255;
  }
  double* F(char* p) const { return reinterpret_cast<double*>(p + factor); }
  double* D(char* p) const { return reinterpret_cast<double*>(p + diag); }
  double* Bs(char* p) const { return reinterpret_cast<double*>(p + base); }
  double* Out(char* p) const { return reinterpret_cast<double*>(p + out); }
  int* Info(char* p) const { return reinterpret_cast<int*>(p + info); }
};
static const double kSampleRungs[4] = {0.0, 1e-8, 1e-7, 1e-6};      // relative to s_y^2: the ladder of cholesky_attempts

// Where a posterior call runs: a context, or the B runs of a batch (run 0's buffers, the others zs bytes apart).  A context is the
// view with one run, every stride 0 and the default AcqBatch, so its launches carry the arguments of a single context.
struct PostSite {
  pcabo_ctx* ctx = nullptr;          // the context asked ...
  pcabo_batch* batch = nullptr;      // ... or the batch: whose error text is written
  pcabo_ctx* c0;                     // the context, or run 0: dXq, dKS and dPartial of the launches
  hipStream_t s; int device, B = 1; size_t zs = 0;
  GpReady ready;                     // the owner's record on whether a call on the conditioned model can go ahead
  int xq_cols;                       // coordinates per staged query: k, or the largest k of the runs
  GpModel m; AcqParams p; AcqBatch ab; double noise;
  char** post_slot; size_t post_v, post_bytes, vzs = 0;   // the runs' V | cov blocks: V's doubles, a block's bytes, the launches' stride
  char** sample_slot; SampleBlock L; size_t szs = 0;      // the runs' sample blocks and the launches' stride
  hipMemcpyKind in = hipMemcpyHostToDevice, out = hipMemcpyDeviceToHost;

  PostSite(pcabo_ctx* run0, int max_q, char** post, char** sample)      // both views: V (NPcap x max_q), cov (max_q^2) behind it
      : c0(run0), post_slot(post), post_v((size_t)run0->lay.s.NPcap * run0->max_q),
        post_bytes(((post_v + (size_t)max_q * max_q) * sizeof(double) + 255) & ~(size_t)255), sample_slot(sample), L(max_q) {}
  explicit PostSite(pcabo_ctx* c) : PostSite(c, c->max_q, &c->dPostV, &c->dSample) {
    ctx = c; s = c->stream; device = c->device; ready = c->st.gp_ready(); xq_cols = c->st.k; noise = c->st.noise;
    m = gp_model(c); p = make_params(c, 0.0, 1, PCABO_ACQ_UCB, 0);      // (the kernels read 1 / lengthscale and the kernel code)
    if (c->ptr_mode != PCABO_PTR_HOST) in = out = hipMemcpyDeviceToDevice;
  }
  explicit PostSite(pcabo_batch* b) : PostSite(b->ctx[0], b->max_q, &b->dPost, &b->dSample) {
    batch = b; s = b->stream; device = b->device; B = b->B; zs = b->zs; vzs = post_bytes; szs = L.bytes; noise = b->st.m.noise;
    ready = b->st.gp_ready(); xq_cols = batch_max_k(b);
    m = gp_model(b, xq_cols); p = batch_params(b, 1, PCABO_ACQ_UCB, 0); ab = batch_ab(b, 0, 0);
  }
  int fail(int code, const char* fmt, const char* a = "", int v = 0) const {
    return batch ? bset_err(batch, code, fmt, a, v) : set_err(ctx, code, fmt, a, v);
  }
  bool live(int b) const { return !batch || (batch->active[b] && batch->ctx[b]->st.conditioned()); }   // is run b's result handed out?
  double* V() const { return reinterpret_cast<double*>(*post_slot); }
  double* cov(int b = 0) const { return reinterpret_cast<double*>(*post_slot + (size_t)b * post_bytes) + post_v; }
  char* blk(int b = 0) const { return *sample_slot + (size_t)b * L.bytes; }
  // mean | variance | unfloored variance of a call with q queries, in dPartial behind the records of the scoring
  double* post(int q) const { return c0->dPartial + partial_post_result(q, m.NP).start; }
};
#define PHIPCHK(call)                                                                                           \
  do {                                                                                                          \
    hipError_t e_ = (call);                                                                                     \
    if (e_ != hipSuccess) return w.fail(PCABO_ERR_HIP, "HIP error: %s (line %d)", hipGetErrorString(e_), __LINE__); \
  } while (0)

// The state every call on a conditioned model needs: nothing of the context or the batch in flight, and a GP to ask.
static int post_state_check(const PostSite& w, const char* name) {
  if (w.ready == GP_IN_FLIGHT)
    return w.fail(PCABO_ERR_ARG, w.batch ? "%s: a conditioning or a _begin call of this batch has not been ended"
                                         : "%s: a conditioning is in flight, call pcabo_gp_condition_end first", name);
  if (w.ready == GP_NONE) return w.fail(PCABO_ERR_ARG, w.batch ? "%s: no conditioned GP" : "%s: no conditioned GP, call pcabo_gp_condition first", name);
  return PCABO_OK;
}

// The query of `name` on its way: state checks, the V | cov blocks and the sample blocks on their first use, Xq staged, the
// launches.  want_cov: with V and the covariance; want_samples: the sample blocks exist afterwards.
static int post_enqueue(const PostSite& w, const char* name, const double* Xq, int q, int flags, bool want_cov, bool want_samples) {
  if (const int rc = post_state_check(w, name)) return rc;
  PHIPCHK(hipSetDevice(w.device));
  if (want_cov && !*w.post_slot) PHIPCHK(hipMalloc((void**)w.post_slot, w.post_bytes * (size_t)w.B));
  if (want_samples && !*w.sample_slot) PHIPCHK(hipMalloc((void**)w.sample_slot, w.L.bytes * (size_t)w.B));
  if (w.batch)
    PHIPCHK(hipMemcpy2DAsync(w.c0->dXq, w.zs, Xq, (size_t)q * w.batch->max_d * sizeof(double), (size_t)q * w.xq_cols * sizeof(double),
                             w.B, w.in, w.s));
  else
    PHIPCHK(hipMemcpyAsync(w.c0->dXq, Xq, (size_t)q * w.xq_cols * sizeof(double), w.in, w.s));
  launch_posterior(w.s, w.c0->dXq, q, w.m, w.p, w.noise, flags & PCABO_POST_OBS_NOISE, w.c0->dKS, w.c0->dPartial, w.post(q),
                   want_cov ? w.V() : nullptr, want_cov ? w.cov() : nullptr, w.ab, w.vzs, w.B);
  return PCABO_OK;
}

// One rung for zb.B runs (blk: the first one's block, zb.zs: the block stride): prep from the untouched cov, the factorisation, the
// info words on their way to the host.  PCABO_OK, or PCABO_ERR_HIP when nothing could be launched.
static int sample_factor_enqueue(hipStream_t s, const SampleBlock& L, char* blk, const double* cov, const double* ystats, int q,
                                 double jitter, size_t zs, size_t vzs, ZB zb, int* info_host) {
  const int QP = round_up(q, PCABO_BS);
  launch_post_chol_prep(s, cov, q, ystats, jitter, L.F(blk), L.Info(blk), zs, vzs, zb.zs, zb.B);
  if (launch_cholesky(s, L.F(blk), QP, QP, L.Info(blk), L.D(blk), zb) != 0) return PCABO_ERR_HIP;
  const hipError_t e = zb.B > 1 ? hipMemcpy2DAsync(info_host, sizeof(int), L.Info(blk), zb.zs, sizeof(int), zb.B, hipMemcpyDeviceToHost, s)
                                : hipMemcpyAsync(info_host, L.Info(blk), sizeof(int), hipMemcpyDeviceToHost, s);
  return e == hipSuccess ? PCABO_OK : PCABO_ERR_HIP;
}

// The query with its covariance, the base samples staged, then the jitter ladder: the first rung as one launch sequence for all
// runs; a live run whose info word is not 0 climbs the other rungs alone on its own block, with the launches of a single context.
// rung[b]: the rung that could be factored (0 .. 3), -1 when none could or the run is not live.
static int sample_enqueue(const PostSite& w, const char* name, const double* Xq, int q, int flags, const double* base, int S, int* rung) {
  if (const int rc = post_enqueue(w, name, Xq, q, flags, true, true)) return rc;
  const SampleBlock& L = w.L;
  const size_t row = (size_t)S * q * sizeof(double);
  if (w.batch) PHIPCHK(hipMemcpy2DAsync(L.Bs(w.blk()), L.bytes, base, row, row, w.B, w.in, w.s));
  else PHIPCHK(hipMemcpyAsync(L.Bs(w.blk()), base, row, w.in, w.s));
  std::vector<int> info((size_t)w.B, -1);
  ZB zb; zb.B = w.B; zb.zs = w.szs;
  if (sample_factor_enqueue(w.s, L, w.blk(), w.cov(), w.m.ystats, q, kSampleRungs[0], w.zs, w.vzs, zb, info.data()) != PCABO_OK)
    return w.fail(PCABO_ERR_HIP, "%s: the factorisation could not be launched", name);
  PHIPCHK(wait_stream(w.s));
  for (int b = 0; b < w.B; ++b) {
    rung[b] = w.live(b) && info[b] == 0 ? 0 : -1;
    const double* ystats_b = reinterpret_cast<const double*>(reinterpret_cast<const char*>(w.m.ystats) + (size_t)b * w.zs);
    for (int r = 1; r < 4 && w.live(b) && rung[b] < 0; ++r) {
      if (sample_factor_enqueue(w.s, L, w.blk(b), w.cov(b), ystats_b, q, kSampleRungs[r], 0, 0, ZB(), &info[b]) != PCABO_OK)
        return w.fail(PCABO_ERR_HIP, "%s: the factorisation could not be launched", name);
      PHIPCHK(wait_stream(w.s));
      if (info[b] == 0) rung[b] = r;
    }
  }
  return PCABO_OK;
}
// ... and the product behind it, for all runs
static void sample_product(const PostSite& w, int q, int flags, int S) {
  launch_post_sample(w.s, w.L.F(w.blk()), q, w.L.Bs(w.blk()), S, (flags & PCABO_POST_CENTRED) ? nullptr : w.post(q), w.L.Out(w.blk()),
                     w.zs, w.szs, w.B);
}

// A context copies straight from the device to the caller's arrays (device pointers in PCABO_PTR_DEVICE mode).
int pcabo_gp_posterior(pcabo_ctx* ctx, const double* Xq, int q, int flags, double* mean, double* var, double* cov) {
  if (!ctx) return PCABO_ERR_ARG;
  if (const char* why = post_arg_error(Xq, q, ctx->max_q, flags, mean || var || cov))
    return set_err(ctx, PCABO_ERR_ARG, "pcabo_gp_posterior: %s", why);
  const PostSite w(ctx);
  if (const int rc = post_enqueue(w, "pcabo_gp_posterior", Xq, q, flags, cov != nullptr, false)) return rc;
  double* post = w.post(q);
  if (mean) PHIPCHK(hipMemcpyAsync(mean, post, (size_t)q * sizeof(double), w.out, w.s));
  if (var) PHIPCHK(hipMemcpyAsync(var, post + q, (size_t)q * sizeof(double), w.out, w.s));
  if (cov) PHIPCHK(hipMemcpyAsync(cov, w.cov(), (size_t)q * q * sizeof(double), w.out, w.s));
  PHIPCHK(wait_stream(w.s));
  PHIPCHK(hipGetLastError());
  return PCABO_OK;
}

int pcabo_gp_posterior_sample(pcabo_ctx* ctx, const double* Xq, int q, int flags, const double* base, int S, double* samples,
                              double* mean, double* jitter_used) {
  if (!ctx) return PCABO_ERR_ARG;
  if (const char* why = sample_arg_error(Xq, q, ctx->max_q, flags, base, S, samples))
    return set_err(ctx, PCABO_ERR_ARG, "pcabo_gp_posterior_sample: %s", why);
  const PostSite w(ctx);
  int rung = -1;
  if (const int rc = sample_enqueue(w, "pcabo_gp_posterior_sample", Xq, q, flags, base, S, &rung)) return rc;
  if (rung < 0)
    return set_err(ctx, PCABO_ERR_NOT_PD, "pcabo_gp_posterior_sample: the posterior covariance of the %s%d queries is not positive definite after the jitter retries", "", q);
  sample_product(w, q, flags, S);
  PHIPCHK(hipMemcpyAsync(samples, w.L.Out(w.blk()), (size_t)S * q * sizeof(double), w.out, w.s));
  if (mean) PHIPCHK(hipMemcpyAsync(mean, w.post(q), (size_t)q * sizeof(double), w.out, w.s));
  PHIPCHK(wait_stream(w.s));
  PHIPCHK(hipGetLastError());
  if (jitter_used) *jitter_used = kSampleRungs[rung];
  return PCABO_OK;
}

// A batch gathers mean / variance of all runs with one 2-D copy and hands out only the live runs' results.
int pcabo_batch_gp_posterior(pcabo_batch* batch, const double* Xq, int q, int flags, double* mean, double* var, double* cov, int* status) {
  if (!batch) return PCABO_ERR_ARG;
  if (const char* why = post_arg_error(Xq, q, batch->max_q, flags, mean || var || cov))
    return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_gp_posterior: %s", why);
  const PostSite w(batch);
  if (const int rc = post_enqueue(w, "pcabo_batch_gp_posterior", Xq, q, flags, cov != nullptr, false)) return rc;
  const int B = w.B;
  std::vector<double> mv((size_t)B * 2 * q);
  PHIPCHK(hipMemcpy2DAsync(mv.data(), (size_t)2 * q * sizeof(double), w.post(q), w.zs, (size_t)2 * q * sizeof(double), B, w.out, w.s));
  for (int b = 0; b < B; ++b) {
    if (status) status[b] = w.live(b) ? PCABO_OK : PCABO_ERR_ARG;
    if (w.live(b) && cov) PHIPCHK(hipMemcpyAsync(cov + (size_t)b * q * q, w.cov(b), (size_t)q * q * sizeof(double), w.out, w.s));
  }
  PHIPCHK(wait_stream(w.s));
  PHIPCHK(hipGetLastError());
  for (int b = 0; b < B; ++b) {
    if (!w.live(b)) continue;
    if (mean) memcpy(mean + (size_t)b * q, &mv[(size_t)b * 2 * q], (size_t)q * sizeof(double));
    if (var) memcpy(var + (size_t)b * q, &mv[(size_t)b * 2 * q + q], (size_t)q * sizeof(double));
  }
  return PCABO_OK;
}

int pcabo_batch_gp_posterior_sample(pcabo_batch* batch, const double* Xq, int q, int flags, const double* base, int S, double* samples,
                                    double* mean, double* jitter_used, int* status) {
  if (!batch) return PCABO_ERR_ARG;
  if (const char* why = sample_arg_error(Xq, q, batch->max_q, flags, base, S, samples))
    return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_gp_posterior_sample: %s", why);
  const PostSite w(batch);
  const int B = w.B;
  std::vector<int> rung((size_t)B, -1);
  if (const int rc = sample_enqueue(w, "pcabo_batch_gp_posterior_sample", Xq, q, flags, base, S, rung.data())) return rc;
  sample_product(w, q, flags, S);
  std::vector<double> mv(mean ? (size_t)B * q : 0);
  if (mean) PHIPCHK(hipMemcpy2DAsync(mv.data(), (size_t)q * sizeof(double), w.post(q), w.zs, (size_t)q * sizeof(double), B, w.out, w.s));
  for (int b = 0; b < B; ++b) {
    if (status) status[b] = rung[b] >= 0 ? PCABO_OK : w.live(b) ? PCABO_ERR_NOT_PD : PCABO_ERR_ARG;
    if (rung[b] >= 0)
      PHIPCHK(hipMemcpyAsync(samples + (size_t)b * S * q, w.L.Out(w.blk(b)), (size_t)S * q * sizeof(double), w.out, w.s));
  }
  PHIPCHK(wait_stream(w.s));
  PHIPCHK(hipGetLastError());
  for (int b = 0; b < B; ++b) {
    if (rung[b] < 0) continue;
    if (mean) memcpy(mean + (size_t)b * q, &mv[(size_t)b * q], (size_t)q * sizeof(double));
    if (jitter_used) jitter_used[b] = kSampleRungs[rung[b]];
  }
  return PCABO_OK;
}

// ---- leave-one-out predictions (DESIGN.md "Leave-one-out predictions") ----------------------------------------------------------
// One launch of k_loo for the context or for all runs of the batch: it reads R, alpha, y_s and the Standardize statistics where the
// conditioning (or the fit) left them and writes mean | var | z | lpd, 4 n doubles per run, to the head of dPartial, which every
// evaluation writes before it reads.  Nothing else is touched: no sequence number, no ticket, no second stream.  The results are
// host arrays in either pointer mode; lpd_sum is added here, from the n values brought back, in index order.
static int loo_enqueue(const PostSite& w, const char* name, bool any_out) {
  if (!any_out) return w.fail(PCABO_ERR_ARG, "%s: mean, var, z, lpd and lpd_sum are all NULL", name);
  if (const int rc = post_state_check(w, name)) return rc;
  PHIPCHK(hipSetDevice(w.device));
  launch_loo(w.s, w.m.R, w.m.alpha, w.c0->dYs, w.m.ystats, w.m.n, w.m.ld, w.c0->dPartial, w.zs, w.B);
  return PCABO_OK;
}
static double loo_sum(const double* lpd, size_t n) {
  double sum = 0.0;
  for (size_t i = 0; i < n; ++i) sum += lpd[i];
  return sum;
}

int pcabo_gp_loo(pcabo_ctx* ctx, double* mean, double* var, double* z, double* lpd, double* lpd_sum) {
  if (!ctx) return PCABO_ERR_ARG;
  const PostSite w(ctx);
  if (const int rc = loo_enqueue(w, "pcabo_gp_loo", mean || var || z || lpd || lpd_sum)) return rc;
  const size_t n = (size_t)w.m.n;
  std::vector<double> own(lpd_sum && !lpd ? n : 0);      // the sum is asked for without its terms
  double* out[4] = {mean, var, z, lpd ? lpd : lpd_sum ? own.data() : nullptr};
  for (int v = 0; v < 4; ++v)
    if (out[v]) PHIPCHK(hipMemcpyAsync(out[v], w.c0->dPartial + partial_loo_part(w.m.n, v), n * sizeof(double), hipMemcpyDeviceToHost, w.s));
  PHIPCHK(wait_stream(w.s));
  PHIPCHK(hipGetLastError());
  if (lpd_sum) *lpd_sum = loo_sum(out[3], n);
  return PCABO_OK;
}

// A batch gathers the 4 n doubles of every run with one 2-D copy and hands out only the live runs' results.
int pcabo_batch_gp_loo(pcabo_batch* batch, double* mean, double* var, double* z, double* lpd, double* lpd_sum, int* status) {
  if (!batch) return PCABO_ERR_ARG;
  const PostSite w(batch);
  if (const int rc = loo_enqueue(w, "pcabo_batch_gp_loo", mean || var || z || lpd || lpd_sum)) return rc;
  const int B = w.B;
  const size_t n = (size_t)w.m.n;
  const size_t n4 = partial_loo(w.m.n).count;
  std::vector<double> all((size_t)B * n4);
  PHIPCHK(hipMemcpy2DAsync(all.data(), n4 * sizeof(double), w.c0->dPartial, w.zs, n4 * sizeof(double), B, hipMemcpyDeviceToHost, w.s));
  PHIPCHK(wait_stream(w.s));
  PHIPCHK(hipGetLastError());
  double* out[4] = {mean, var, z, lpd};
  for (int b = 0; b < B; ++b) {
    if (status) status[b] = w.live(b) ? PCABO_OK : PCABO_ERR_ARG;
    if (!w.live(b)) continue;
    const double* run = &all[(size_t)b * n4];
    for (int v = 0; v < 4; ++v)
      if (out[v]) memcpy(out[v] + (size_t)b * n, run + partial_loo_part(w.m.n, v), n * sizeof(double));
    if (lpd_sum) lpd_sum[b] = loo_sum(run + partial_loo_part(w.m.n, 3), n);
  }
  return PCABO_OK;
}

}  // extern "C" (helpers with C++ linkage follow)
// ---- appending points to the conditioned GP and taking them back (DESIGN.md "Extending a conditioned GP", "Extending the GPs of a
// batch"): ONE host sequence for a single context and for the B runs of a batch -------------------------------------------------
// The fantasy model of botorch's condition_on_observations: transforms and hyperparameters held, only the data grow.  Per point
// k_ext_ks, v = R ks and w = R^T v (launch_alpha's two launches on the kernel vector) and k_ext_append (kernels_ext.hip); behind the
// last point (believer mode: behind every point, the next one reads the mean) alpha on the grown y_s, then ONE copy of the info
// word(s) and one wait.  A pivot that fails stops the writes of everything behind it on the device; the host then takes the call
// back with truncate's launches.  Of the state that later calls read, n, NP, L, R, ZnT, AT, nrm, y_s and alpha change, the tickets
// are reset where NP changes and the transposed root inverse of the device-resident optimiser is marked stale.
// A batch: the same launches for all runs at once (blockIdx.z = run), every run with its own header {rung, info word}; a run that
// takes no part (parked, without a GP, set aside) gets the info word EXT_INFO_SKIP and is left alone by the kernels of
// kernels_ext.hip and by the gated form of launch_alpha.  A run whose pivot failed is taken back alone, as one run on its own
// buffers, and is then SET ASIDE (model_state.h) until a truncate reaches the n it holds.
struct ExtHeader { double rung; int info, pad; };
static_assert(sizeof(ExtHeader) == EXT_HDR * sizeof(double), "the header the kernels of kernels_ext.hip read");

// What an extension needs beyond the posterior call's site.  A plain or a strided copy, launch_alpha or its gated form: by owner
// (zs, gate), never by B == 1 - a batch of one run keeps its header with EXT_INFO_SKIP, the gated alpha and its strided copies.
struct ExtSite {
  const PostSite& w;                 // the owner: its stream, model and parameters; whose error text is written
  pcabo_ctx* c;                      // whose buffers the launches name: the context, run 0 of a batch, or a member taken back alone
  ExtScratch e; GpArrays a;          // the scratch at the head of c's dPartial; the arrays the kernels write
  int k, B = 1; size_t zs = 0; AcqBatch ab; ZB zb;      // (a batch: the widest run's k, every run reads its own from ab.k_dev)
  const int* gate = nullptr;         // a batch: run 0's gate word, which is the info word of its header
  std::vector<char> go;              // who takes part (a context: itself)
  ExtSite(const PostSite& site, pcabo_ctx* own)      // one run on its own buffers: the launches of a single context
      : w(site), c(own), e(own->dPartial, own->lay.s), a(gp_arrays(own)), k(own->st.k), go(1, 1) {}
  explicit ExtSite(const PostSite& site) : ExtSite(site, site.c0) {
    if (!site.batch) return;
    k = site.xq_cols; B = site.B; zs = site.zs; ab = site.ab; zb = batch_zb(site.batch); gate = info_word(); go.assign((size_t)B, 0);
  }
  int* info_word() const { return reinterpret_cast<int*>(e.small + EXT_HDR_INFO); }
  pcabo_ctx* run(int b) const { return gate ? w.batch->ctx[b] : c; }
};

static GpModel ext_model(const PostSite& w, int n) { GpModel m = w.m; m.n = n; m.NP = round_up(n, PCABO_BS); return m; }
static bool all_finite(const double* v, size_t n) { return std::all_of(v, v + n, [](double t) { return std::isfinite(t); }); }

// What an extend refuses whoever owns the model: the text behind the entry point's name (%d: max_n), or null.  The counts mean
// something only where a GP stands: without one, post_state_check behind this refuses the call.
static const char* ext_arg_error(const PostSite& w, const double* Zp, const double* yp, int p, int flags, int n, int max_n) {
  if (!Zp) return "%s: Zp is required";
  if (flags & ~PCABO_EXTEND_BELIEVER) return "%s: unknown flag bits";
  if (!yp && !(flags & PCABO_EXTEND_BELIEVER)) return "%s: yp is required without PCABO_EXTEND_BELIEVER";
  if (p < 1) return "%s: p must be at least 1";
  if (w.ready != GP_READY) return nullptr;
  if (n + p > max_n) return "%s: n + p exceeds max_n (%d)";
  if ((round_up(n + p, PCABO_BS) + 255) / 256 > EXT_MU_MAX) return "%s: n + p beyond what the kernels cover";
  return nullptr;
}

// The header(s) on their way: every run's rung, the info word cleared where the run takes part and EXT_INFO_SKIP elsewhere.
// hdr (x.B of them) lives until the caller has waited for the stream.
static int ext_put_headers(const ExtSite& x, ExtHeader* hdr) {
  const PostSite& w = x.w;
  for (int b = 0; b < x.B; ++b) hdr[b] = ExtHeader{x.run(b)->st.rung, x.go[b] ? 0 : EXT_INFO_SKIP, 0};
  if (x.zs) PHIPCHK(hipMemcpy2DAsync(x.e.small + EXT_HDR_RUNG, x.zs, hdr, sizeof(ExtHeader), sizeof(ExtHeader), x.B, hipMemcpyHostToDevice, w.s));
  else PHIPCHK(hipMemcpyAsync(x.e.small + EXT_HDR_RUNG, hdr, sizeof(ExtHeader), hipMemcpyHostToDevice, w.s));
  return PCABO_OK;
}

// The per-query tickets are consistent only with acq_slabs(NP): where NP changes outside a conditioning they are reset as
// enqueue_rows_dh resets them - a batch's those of ALL runs, where its record or a member's asks.
static int ext_tickets(const ExtSite& x) {
  const PostSite& w = x.w;
  const bool reset = w.batch ? w.batch->st.tickets_reset_if_needed(acq_slabs(w.batch->st.m.NP), w.batch->run_st)
                             : w.ctx->st.tickets_reset_if_needed(acq_slabs(w.ctx->st.NP));
  if (!reset) return PCABO_OK;
  if (x.zs) PHIPCHK(hipMemset2DAsync(x.c->dCounters, x.zs, 0, ticket_bytes(x.c), x.B, w.s));
  else PHIPCHK(hipMemsetAsync(x.c->dCounters, 0, ticket_bytes(x.c), w.s));
  return PCABO_OK;
}

// out = R^T (R y) on n points - the conditioning's own launches, or their gated form with the site's gate word
static void ext_rtr(const ExtSite& x, const double* y, int n, double* tmp, double* out) {
  if (x.gate) launch_alpha_gated(x.w.s, x.c->dR, y, n, round_up(n, PCABO_BS), x.c->ld, tmp, out, x.zb, x.gate);
  else launch_alpha(x.w.s, x.c->dR, y, n, round_up(n, PCABO_BS), x.c->ld, tmp, out);
}
static void ext_alpha(const ExtSite& x, int n) { ext_rtr(x, x.c->dYs, n, x.c->dTmp, x.c->dAlpha); }

static int ext_wait(const PostSite& w) {
  PHIPCHK(wait_stream(w.s));
  PHIPCHK(hipGetLastError());
  return PCABO_OK;
}

// p points appended behind the n0 there are: the header(s), then at most rows_cap points at a time (those that fit dXq with their
// values, at the widest k).  stage(i0, rows, vals) puts rows i0 .. of every run at the head of its dXq and, where values are given,
// their values vals doubles behind - the one step that differs between the owners.  record() is the owner's side of the new n: the
// counts, then ext_tickets.  Behind it alpha, the info word(s) to info (x.B of them) with one copy, one wait.
template <class Stage, class Record>
static int ext_append(const ExtSite& x, ExtHeader* hdr, int n0, int p, bool believer, bool values, int* info, Stage&& stage,
                      Record&& record) {
  const PostSite& w = x.w;
  if (const int rc = ext_put_headers(x, hdr)) return rc;
  const int rows_cap = ext_rows_cap(x.c->lay.s, w.xq_cols);
  const size_t vals = xq_ext_vals(x.c->lay.s, w.xq_cols).start;
  double* dY = values ? x.c->dXq + vals : nullptr;
  int n = n0;
  for (int i0 = 0; i0 < p; i0 += rows_cap) {
    const int rows = std::min(rows_cap, p - i0);
    if (const int rc = stage(i0, rows, vals)) return rc;
    for (int i = 0; i < rows; ++i, ++n) {
      const GpModel m = ext_model(w, n);
      launch_ext_ks(w.s, x.c->dXq, i, dY, i, m, w.p.inv_ls, w.p.kernel, x.e, x.ab, x.B);
      ext_rtr(x, x.e.ks, n, x.e.v, x.e.w);
      launch_ext_append(w.s, m, x.e, i0 + i, believer ? 1 : 0, w.noise, w.p.inv_ls, x.a, x.ab, x.B);
      if (believer && i0 + i + 1 < p) ext_alpha(x, n + 1);
    }
  }
  if (const int rc = record()) return rc;
  ext_alpha(x, n);
  if (x.zs) PHIPCHK(hipMemcpy2DAsync(info, sizeof(int), x.info_word(), x.zs, sizeof(int), x.B, hipMemcpyDeviceToHost, w.s));
  else PHIPCHK(hipMemcpyAsync(info, x.info_word(), sizeof(int), hipMemcpyDeviceToHost, w.s));
  return ext_wait(w);
}

// Points n0 .. of the n_now there are go: the header(s), k_ext_truncate, and alpha on n0 points behind record(), the owner's side
// of the changed n (a member of a batch taken back alone: none here, its batch follows it up).  The caller waits.
template <class Record>
static int ext_take_back(const ExtSite& x, ExtHeader* hdr, int n0, int n_now, Record&& record) {
  if (const int rc = ext_put_headers(x, hdr)) return rc;
  launch_ext_truncate(x.w.s, x.e, n0, x.k, round_up(n_now, PCABO_BS), x.c->ld, x.a, x.ab, x.B);
  if (const int rc = record()) return rc;
  ext_alpha(x, n0);
  return PCABO_OK;
}

extern "C" {
// A context copies the points straight from the caller's arrays (device pointers in PCABO_PTR_DEVICE mode).
int pcabo_gp_extend(pcabo_ctx* ctx, const double* Zp, const double* yp, int p, int flags) {
  if (!ctx) return PCABO_ERR_ARG;
  const char* name = "pcabo_gp_extend";
  if (ctx->in_batch) return set_err(ctx, PCABO_ERR_ARG, "%s: the context belongs to a batch", name);      // (its lock-step form: pcabo_batch_gp_extend)
  const PostSite w(ctx);
  const int n0 = ctx->st.n, k = ctx->st.k;
  if (const char* why = ext_arg_error(w, Zp, yp, p, flags, n0, ctx->max_n)) return w.fail(PCABO_ERR_ARG, why, name, ctx->max_n);
  if (const int rc = post_state_check(w, name)) return rc;
  const bool believer = (flags & PCABO_EXTEND_BELIEVER) != 0;
  if (believer) yp = nullptr;
  if (w.in == hipMemcpyHostToDevice) {                 // host pointers: every coordinate and value
    if (!all_finite(Zp, (size_t)p * k)) return w.fail(PCABO_ERR_ARG, "%s: a coordinate is not finite", name);
    if (yp && !all_finite(yp, (size_t)p)) return w.fail(PCABO_ERR_ARG, "%s: a value is not finite", name);
  }
  PHIPCHK(hipSetDevice(w.device));
  const ExtSite x(w);
  const auto set_n = [&](int n) { ctx->st.n_changed(n); return ext_tickets(x); };
  ExtHeader hdr;
  int fail = 0;
  const int rc = ext_append(x, &hdr, n0, p, believer, yp != nullptr, &fail, [&](int i0, int rows, size_t vals) -> int {
    PHIPCHK(hipMemcpyAsync(ctx->dXq, Zp + (size_t)i0 * k, (size_t)rows * k * sizeof(double), w.in, w.s));
    if (yp) PHIPCHK(hipMemcpyAsync(ctx->dXq + vals, yp + i0, (size_t)rows * sizeof(double), w.in, w.s));
    return PCABO_OK;
  }, [&] { return set_n(n0 + p); });
  if (rc || fail == 0) return rc;
  if (const int rc = ext_take_back(x, &hdr, n0, n0 + p, [&] { return set_n(n0); })) return rc;
  if (const int rc = ext_wait(w)) return rc;
  return w.fail(PCABO_ERR_NOT_PD, "%s: the bordered matrix is not positive definite at new point %d; the call has been taken back", name, fail - 1);
}

int pcabo_gp_truncate(pcabo_ctx* ctx, int n0) {
  if (!ctx) return PCABO_ERR_ARG;
  const char* name = "pcabo_gp_truncate";
  if (ctx->in_batch) return set_err(ctx, PCABO_ERR_ARG, "%s: the context belongs to a batch", name);      // (its lock-step form: pcabo_batch_gp_truncate)
  const PostSite w(ctx);
  if (const int rc = post_state_check(w, name)) return rc;
  const int n = ctx->st.n;
  if (n0 < ctx->st.n_base || n0 > n) return w.fail(PCABO_ERR_ARG, "%s: n0 must lie in n_base .. n", name);
  if (n0 == n) return PCABO_OK;
  PHIPCHK(hipSetDevice(w.device));
  const ExtSite x(w);
  ExtHeader hdr;
  if (const int rc = ext_take_back(x, &hdr, n0, n, [&] { ctx->st.n_changed(n0); return ext_tickets(x); })) return rc;
  return ext_wait(w);
}

int pcabo_gp_extended(pcabo_ctx* ctx, int* n_base, int* n) {
  if (!ctx) return PCABO_ERR_ARG;
  if (n_base) *n_base = ctx->st.n_base;
  if (n) *n = ctx->st.n;
  return PCABO_OK;
}

// A batch packs the points of the runs that take part through their pinned hXq (which is waited for when the staging goes round
// again: rare, p beyond rows_cap) and sends them with one strided copy.
int pcabo_batch_gp_extend(pcabo_batch* batch, const double* Zp, const double* yp, int p, int flags, int* status) {
  if (!batch) return PCABO_ERR_ARG;
  const char* name = "pcabo_batch_gp_extend";
  const PostSite w(batch);
  const int B = w.B, n0 = batch->st.m.n, MD = batch->max_d;
  if (const char* why = ext_arg_error(w, Zp, yp, p, flags, n0, batch->max_n)) return w.fail(PCABO_ERR_ARG, why, name, batch->max_n);
  if (const int rc = post_state_check(w, name)) return rc;
  const bool believer = (flags & PCABO_EXTEND_BELIEVER) != 0;
  if (believer) yp = nullptr;
  ExtSite x(w);
  for (int b = 0; b < B; ++b) {                        // every coordinate and value of the runs that take part; the others' are not read
    if (!(x.go[b] = w.live(b))) continue;                 // (active and conditioned: not parked, without a GP or set aside)
    if (!all_finite(Zp + (size_t)b * p * MD, (size_t)p * batch->ctx[b]->st.k))
      return w.fail(PCABO_ERR_ARG, "%s: a coordinate of run %d is not finite", name, b);
    if (yp && !all_finite(yp + (size_t)b * p, (size_t)p)) return w.fail(PCABO_ERR_ARG, "%s: a value of run %d is not finite", name, b);
  }
  PHIPCHK(hipSetDevice(w.device));
  const int n = n0 + p;
  std::vector<ExtHeader> hdr((size_t)B);
  std::vector<int> info((size_t)B, 0);
  const int rc = ext_append(x, hdr.data(), n0, p, believer, yp != nullptr, info.data(), [&](int i0, int rows, size_t vals) -> int {
    if (i0 > 0) PHIPCHK(wait_stream(w.s));
    for (int b = 0; b < B; ++b) {
      if (!x.go[b]) continue;
      pcabo_ctx* c = batch->ctx[b];
      const int k = c->st.k;
      memcpy(c->hXq, Zp + (size_t)b * p * MD + (size_t)i0 * k, (size_t)rows * k * sizeof(double));
      if (yp) memcpy(c->hXq + vals, yp + (size_t)b * p + i0, (size_t)rows * sizeof(double));
    }
    const size_t staged = yp ? vals + (size_t)rows : (size_t)rows * w.xq_cols;
    PHIPCHK(hipMemcpy2DAsync(x.c->dXq, w.zs, x.c->hXq, batch->hzs, staged * sizeof(double), B, hipMemcpyHostToDevice, w.s));
    return PCABO_OK;
  }, [&] { batch->st.points_appended(p); return ext_tickets(x); });
  if (rc) return rc;
  // the runs whose pivot failed: each alone back to the bytes of entry; its record follows below
  int failed = 0, first_bad = -1, first_point = 0;
  for (int b = 0; b < B; ++b) {
    if (!x.go[b] || info[b] <= 0) continue;
    if (const int rc = ext_take_back(ExtSite(w, batch->ctx[b]), &hdr[b], n0, n, [] { return (int)PCABO_OK; })) return rc;
    if (!failed++) { first_bad = b; first_point = info[b] - 1; }
  }
  if (failed)
    if (const int rc = ext_wait(w)) return rc;
  for (int b = 0; b < B; ++b) {
    pcabo_ctx* c = batch->ctx[b];
    const bool ok = x.go[b] && info[b] == 0;
    c->st.follow_extend(batch->st, ok, n0);
    if (status) status[b] = ok ? PCABO_OK : x.go[b] ? PCABO_ERR_NOT_PD : PCABO_ERR_ARG;
  }
  if (failed) {
    snprintf(batch->err, sizeof(batch->err), "%s: run %d: the bordered matrix is not positive definite at new point %d; %d run(s) "
             "taken back and set aside until pcabo_batch_gp_truncate", name, first_bad, first_point, failed);
  }
  return PCABO_OK;
}

int pcabo_batch_gp_truncate(pcabo_batch* batch, int n0, int* status) {
  if (!batch) return PCABO_ERR_ARG;
  const char* name = "pcabo_batch_gp_truncate";
  const PostSite w(batch);
  if (const int rc = post_state_check(w, name)) return rc;
  const int B = w.B, n = batch->st.m.n;
  if (!batch->st.can_truncate_to(n0)) return w.fail(PCABO_ERR_ARG, "%s: n0 must lie in n_base .. n", name);
  // who holds rows beyond n0: a live run (n of them), a run set aside that this call brings back (aside_n of them)
  ExtSite x(w);
  bool any = false;
  for (int b = 0; b < B; ++b) any = (x.go[b] = batch->ctx[b]->st.own().rows_beyond(n0, n)) || any;
  const auto record = [&] { batch->st.points_taken_back(n0); return ext_tickets(x); };
  if (any) {
    PHIPCHK(hipSetDevice(w.device));
    std::vector<ExtHeader> hdr((size_t)B);
    if (const int rc = ext_take_back(x, hdr.data(), n0, n, record)) return rc;
    if (const int rc = ext_wait(w)) return rc;
  } else if (n0 < n) {
    PHIPCHK(hipSetDevice(w.device));
    if (const int rc = record()) return rc;
    if (const int rc = ext_wait(w)) return rc;
  }
  for (int b = 0; b < B; ++b) {
    pcabo_ctx* c = batch->ctx[b];
    c->st.follow_truncate(batch->st, n0);
    if (status) status[b] = w.live(b) ? PCABO_OK : PCABO_ERR_ARG;
  }
  return PCABO_OK;
}

int pcabo_batch_gp_extended(pcabo_batch* batch, int* n_base, int* n) {
  if (!batch) return PCABO_ERR_ARG;
  if (n_base) *n_base = batch->st.m.n_base;
  if (n) *n = batch->st.m.n;
  return PCABO_OK;
}
#undef PHIPCHK

// a run's status at the start of an optimise call: parked by the caller, without a GP, or taking part
static int batch_run_status(const pcabo_batch* batch, int b) {
  return !batch->active[b] ? PCABO_ERR_ARG : !batch->ctx[b]->st.conditioned() ? PCABO_ERR_NOT_PD : PCABO_OK;
}

// ---- pcabo_batch_optimize_acqf with PCABO_OPT_DEVICE_LBFGSB: every restart group's L-BFGS-B inside one launch of k_lbfgsb_group
// (value 1: device_opt_enqueue / device_opt_collect), or the host's L-BFGS-B over the same kernel's evaluation-only mode, one launch
// per round (value 2, batch_optimize_twin: the twin the device stepping is compared with).

// Does the call qualify (the kernel's size limits, room for its points and records in the runs' buffers - opt_fits, ctx_layout.h -
// finite ordered bounds of every run that takes part)?  act: those runs.  A call that does not takes the host-paced path.
static bool device_opt_eligible(const pcabo_batch* batch, int num_restarts, int batch_limit, const double* bounds, int maxiter,
                                std::vector<int>* act) {
  const int MD = batch->max_d, kmax = batch_max_k(batch);
  if (!lbfgsb_device_possible(batch->st.m.NP, kmax, batch_limit) || maxiter < 1 ||
      !opt_fits(batch->ctx[0]->lay, num_restarts, opt_groups(num_restarts, batch_limit), kmax))
    return false;
  act->clear();
  for (int b = 0; b < batch->B; ++b) {
    if (batch_run_status(batch, b) != PCABO_OK) continue;
    const int k = batch->ctx[b]->st.k;
    const double* bd = bounds + (size_t)b * 2 * MD;
    for (int j = 0; j < k; ++j)
      if (!std::isfinite(bd[j]) || !std::isfinite(bd[k + j]) || bd[j] > bd[k + j]) return false;
    act->push_back(b);
  }
  return true;
}

// One launch of k_lbfgsb_group over the first nent entries of the pinned table, enqueued on the batch's stream: the transposed root
// inverse of the table's runs where a later conditioning outdated it, the table, the runs' points ([num_restarts x k | lower k |
// upper k], strided over the runs), the kernel, and back the head of dVal up to the end of `back` (the values, or the values and
// the groups' records) and the num_restarts candidates or gradients of every run.  The caller waits for the stream.
static int device_opt_launch(pcabo_batch* batch, int nent, int mode, int num_restarts, int batch_limit, int maxiter, int maximize,
                             int acq, Use back) {
  pcabo_ctx* c0 = batch->ctx[0];
  hipStream_t s = batch->stream;
  const int B = batch->B, kmax = batch_max_k(batch);
  for (int e = 0; e < nent; ++e) {
    pcabo_ctx* c = batch->ctx[batch->hOptTab[e] >> 16];
    if (c->st.rt_stale) { launch_rt_build(s, c->dR, c->st.n, c->st.NP, c->ld, c->dGram); c->st.rt_rebuilt(); }
  }
  BHIPCHK(hipMemcpyAsync(batch->dOptTab, batch->hOptTab, (size_t)nent * sizeof(unsigned), hipMemcpyHostToDevice, s));
  BHIPCHK(hipMemcpy2DAsync(c0->dXq, batch->zs, c0->hXq, batch->hzs, xq_opt_points(num_restarts, kmax).count * sizeof(double), B, hipMemcpyHostToDevice, s));
  if (launch_lbfgsb_group(s, batch->dOptTab, nent, mode, num_restarts, maxiter, gp_model(batch, kmax), c0->dXq, c0->dGram, c0->dBestF,
                          c0->dK, 1.0 / batch->st.m.lengthscale, maximize ? 1 : 0, acq, batch->st.m.kernel, c0->dGrad, c0->dVal, batch->zs,
                          batch_hyp(batch), batch_limit) != 0)
    return bset_err(batch, PCABO_ERR_HIP, "the device-resident optimiser could not be launched%s", "");
  BHIPCHK(hipMemcpy2DAsync(c0->hVal, batch->hzs, c0->dVal, batch->zs, (back.start + back.count) * sizeof(double), B, hipMemcpyDeviceToHost, s));
  BHIPCHK(hipMemcpy2DAsync(c0->hGrad, batch->hzs, c0->dGrad, batch->zs, grad_opt_cands(num_restarts, kmax).count * sizeof(double), B, hipMemcpyDeviceToHost, s));
  BHIPCHK(hipGetLastError());
  return PCABO_OK;
}

// Device mode, first half: the launch table, the runs' starts and bounds, the one launch; the call's shape is kept for _collect.
static int device_opt_enqueue(pcabo_batch* batch, const std::vector<int>& act, const double* ics, int num_restarts, int batch_limit,
                              const double* bounds, int maxiter, int maximize, int acq) {
  const int MD = batch->max_d, ngroups = opt_groups(num_restarts, batch_limit);
  int nent = 0;
  for (size_t blk = 0; blk < act.size(); blk += 8)          // both groups of a run on one XCD (work-groups go round the 8 XCDs)
    for (int gi = 0; gi < ngroups; ++gi)
      for (size_t r = blk; r < std::min(act.size(), blk + 8); ++r) {
        const int q0 = gi * batch_limit;
        batch->hOptTab[nent++] = group_entry(act[r], q0, std::min(batch_limit, num_restarts - q0));
      }
  for (int b : act) {
    pcabo_ctx* c = batch->ctx[b];
    const int k = c->st.k;
    memcpy(c->hXq, ics + (size_t)b * num_restarts * MD, (size_t)num_restarts * k * sizeof(double));
    memcpy(c->hXq + (size_t)num_restarts * k, bounds + (size_t)b * 2 * MD, (size_t)2 * k * sizeof(double));
  }
  if (nent > 0)
    if (const int rc = device_opt_launch(batch, nent, 1, num_restarts, batch_limit, maxiter, maximize, acq, val_opt_records(ngroups))) return rc;
  batch->opt_act = act; batch->st.opt_begun(num_restarts, batch_limit);
  return PCABO_OK;
}

// Device mode, second half: wait, then candidates, values and the kernel's eight counters per restart group to the caller.
static int device_opt_collect(pcabo_batch* batch, int num_restarts, int batch_limit, double* cand, double* vals, int* info, int* failed,
                              int* status) {
  if (!batch->st.opt_matches(num_restarts, batch_limit))
    return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_optimize_acqf_end: no matching _begin before it%s", "");
  const int B = batch->B, MD = batch->max_d, ngroups = opt_groups(num_restarts, batch_limit);
  std::vector<int> run_status(B);
  for (int b = 0; b < B; ++b) run_status[b] = batch_run_status(batch, b);
  batch->st.opt_ended();
  BHIPCHK(wait_stream(batch->stream));
  BHIPCHK(hipGetLastError());
  batch->dbg_groups = ngroups; batch->dbg_branches.clear();
  batch->dbg_group_out.assign((size_t)B * ngroups * 8, 0.0);
  for (int b : batch->opt_act) {
    const pcabo_ctx* c = batch->ctx[b];
    const int k = c->st.k;
    int any_failed = 0;
    std::copy(c->hVal + val_opt_record(0), c->hVal + val_opt_record(ngroups), batch->dbg_group_out.begin() + (size_t)b * ngroups * 8);
    for (int gi = 0; gi < ngroups; ++gi) {
      const double* o = c->hVal + val_opt_record(gi);
      if (info) { int* io = info + ((size_t)b * ngroups + gi) * 4; io[0] = (int)o[0]; io[1] = (int)o[1]; io[2] = (int)o[2]; io[3] = (int)o[3]; }
      if ((int)o[2] == 2) any_failed = 1;
      if ((int)o[4] != 0) run_status[b] = (int)o[4];
      if ((int)o[7] != 0) run_status[b] = PCABO_ERR_TIMEOUT;       // evaluation cap (cannot happen within maxiter / maxls)
    }
    if (run_status[b] == PCABO_ERR_NAN) set_err(batch->ctx[b], PCABO_ERR_NAN, "NaN in acquisition gradient%s", "");
    memcpy(cand + (size_t)b * num_restarts * MD, c->hGrad, (size_t)num_restarts * k * sizeof(double));
    memcpy(vals + (size_t)b * num_restarts, c->hVal, (size_t)num_restarts * sizeof(double));
    if (failed) failed[b] = any_failed;
  }
  for (int b = 0; b < B; ++b) {
    if (failed && batch_run_status(batch, b) != PCABO_OK) failed[b] = 0;
    if (status) status[b] = run_status[b];
  }
  return PCABO_OK;
}

// The twin: host L-BFGS-B (csrc/lbfgsb.cpp), evaluations through mode 0 of the same kernel, one launch and one wait per round
static int batch_optimize_twin(pcabo_batch* batch, const std::vector<int>& act, const double* ics, int num_restarts, int batch_limit,
                               const double* bounds, int maxiter, int maximize, int acq, double* cand, double* vals, int* info,
                               int* failed, int* status) {
  const int B = batch->B, MD = batch->max_d, ngroups = opt_groups(num_restarts, batch_limit);
  std::vector<RunRestarts> runs(B);
  for (int b = 0; b < B; ++b) runs[b].status = batch_run_status(batch, b);
  for (int b : act) {
    pcabo_ctx* c = batch->ctx[b];
    // (the device steps in the 64-lane tree order of lbfgsb.cpp: so does its twin)
    runs[b].init(ics + (size_t)b * num_restarts * MD, bounds + (size_t)b * 2 * MD, num_restarts, batch_limit, c->st.k, maxiter, 1);
    runs[b].bind(c->hXq, c->hVal, c->hGrad);
  }
  int nent = 0;
  auto stage = [&](int b, const RestartGroup& rg) { batch->hOptTab[nent++] = group_entry(b, rg.q0, rg.nq); };
  auto eval = [&]() -> int {
    const int n = nent; nent = 0;
    if (const int rc = device_opt_launch(batch, n, 0, num_restarts, batch_limit, maxiter, maximize, acq, val_opt_records(ngroups))) return rc;
    BHIPCHK(wait_stream(batch->stream));
    BHIPCHK(hipGetLastError());
    return PCABO_OK;
  };
  int rc = run_rounds(runs.data(), act, stage, eval);
  for (int b : act) if (runs[b].status == PCABO_ERR_NAN) set_err(batch->ctx[b], PCABO_ERR_NAN, "NaN in acquisition gradient%s", "");
  if (rc != PCABO_OK) return rc;
  // end points: the groups that did not end on their last evaluated point are evaluated there (mode 0 again)
  std::vector<std::pair<int, const RestartGroup*>> redo;
  for (int b : act) {
    if (runs[b].status != PCABO_OK) continue;
    const int k = batch->ctx[b]->st.k;
    double* cb = cand + (size_t)b * num_restarts * MD;
    runs[b].end_points(cb, vals + (size_t)b * num_restarts, [&](const RestartGroup& rg) {
      memcpy(runs[b].xq + (size_t)rg.q0 * k, cb + (size_t)rg.q0 * k, (size_t)rg.nq * k * sizeof(double));
      stage(b, rg);
      redo.push_back({b, &rg});
    });
  }
  if (nent > 0) {
    rc = eval();
    if (rc != PCABO_OK) return rc;
    for (const auto& [b, rg] : redo)
      std::copy(runs[b].val + rg->q0, runs[b].val + rg->q0 + rg->nq, vals + (size_t)b * num_restarts + rg->q0);
  }
  batch->dbg_groups = ngroups; batch->dbg_group_out.clear();
  batch->dbg_branches.assign((size_t)B * ngroups * LBB_COUNT, 0u);
  for (int b = 0; b < B; ++b) {
    const bool any_failed = runs[b].report(info, (size_t)b * ngroups);
    if (failed) failed[b] = any_failed;
    if (status) status[b] = runs[b].status;
    for (size_t gi = 0; gi < runs[b].grp.size(); ++gi) {
      RestartGroup& rg = runs[b].grp[gi];
      // (endpoint_reevaluated is counted where end_points above handed the group to the end-point launch)
      std::copy(rg.opt.branches(), rg.opt.branches() + LBB_COUNT, batch->dbg_branches.begin() + ((size_t)b * ngroups + gi) * LBB_COUNT);
    }
  }
  return PCABO_OK;
}

// Debug exports, not part of the ABI in include/pcabo.h (tests/test_gpu_lbfgsb_branches.py).  After a twin call
// (PCABO_OPT_DEVICE_LBFGSB = 2) of pcabo_batch_optimize_acqf: the branch counters of lbfgsb.h per (run, restart group), out[B][groups]
// [LBB_COUNT]; returns the number of groups per run, 0 if the last call was no twin call, -1 if cap (in entries) is too small.
extern "C" int pcabo_debug_batch_lbfgsb_branches(pcabo_batch* batch, unsigned* out, int cap) {
  if (!batch || batch->dbg_branches.empty()) return 0;
  if (!out || (size_t)cap < batch->dbg_branches.size()) return -1;
  std::copy(batch->dbg_branches.begin(), batch->dbg_branches.end(), out);
  return batch->dbg_groups;
}
// After a device-mode call (value 1; the blocking call or _end): the eight doubles k_lbfgsb_group writes per (run, restart group) -
// niter, nfev, warnflag, task, status, evaluations, ties, evaluation-cap flag; out[B][groups][8] (zeros for a run that took no part).
extern "C" int pcabo_debug_batch_lbfgsb_device_out(pcabo_batch* batch, double* out, int cap) {
  if (!batch || batch->dbg_group_out.empty()) return 0;
  if (!out || (size_t)cap < batch->dbg_group_out.size()) return -1;
  std::copy(batch->dbg_group_out.begin(), batch->dbg_group_out.end(), out);
  return batch->dbg_groups;
}

// The host-paced optimiser: the batch's worker threads drive the runs' L-BFGS-B, one acquisition launch per gang and round.
static int batch_optimize_host(pcabo_batch* batch, const double* ics, int num_restarts, int batch_limit, const double* bounds,
                               int maxiter, int maximize, int acq, double* cand, double* vals, int* info, int* failed, int* status) {
  const int B = batch->B, MD = batch->max_d, kmax = batch_max_k(batch), G = batch->G;
  const int ngroups = opt_groups(num_restarts, batch_limit);
  BHIPCHK(hipStreamSynchronize(batch->stream));
  pcabo_ctx* c0 = batch->ctx[0];
  const GpModel gm = gp_model(batch, kmax);
  const AcqParams pg = batch_params(batch, maximize, acq, 1), pv = batch_params(batch, maximize, acq, 0);
  std::vector<RunRestarts> runs(B);
  for (int b = 0; b < B; ++b) {
    pcabo_ctx* c = batch->ctx[b];
    runs[b].status = batch_run_status(batch, b);
    if (runs[b].status != PCABO_OK) continue;
    runs[b].init(ics + (size_t)b * num_restarts * MD, bounds + (size_t)b * 2 * MD, num_restarts, batch_limit, c->st.k, maxiter);
    runs[b].bind(c->hXq, c->hVal, c->hGrad);
  }
  std::atomic<int> hip_failed{0};
  const int table_cap = PCABO_QA_MAX * 2;          // 32-bit entries in the QueryArgs slot
  if (((B + G - 1) / G) * num_restarts > table_cap)
    return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_optimize_acqf: too many runs per worker thread for one launch table (%s%d entries)", "", table_cap);
  // One gang = the runs b with b % G == g, driven by worker g on its own stream: advance the gang's restart groups,
  // hand every pending (run, query) to ONE launch, wait for the per-query sequence words, feed the results back.
  auto gang = [&](int g) {
    if (hipSetDevice(batch->device) != hipSuccess) { hip_failed.store(1); return; }
    std::vector<int> mine;
    for (int b = g; b < B; b += G) mine.push_back(b);
    const bool use_group = batch->group_acq && batch_limit <= PCABO_GROUP_Q && acq_group_possible(batch->st.m.NP, kmax);
    hipStream_t st = batch->gstream[g];
    QueryArgs tab;                                   // the launch table (travels in the kernel arguments)
    unsigned* ent = reinterpret_cast<unsigned*>(tab.x);
    int nent = 0;
    // one launch of the table's entries (restart groups, or single queries) and the wait for their flags; empties the table
    auto launch = [&](const AcqParams& p, bool groups) -> bool {
      const unsigned long long seq = batch->seq.fetch_add(1) + 1;
      const int n = nent;
      nent = 0;
      if (groups) {
        if (launch_acq_group(st, &tab, n, c0->hXq, gm, p, c0->dPartial, c0->dCounters + counters_group().start, c0->dVal, c0->dGrad,
                             c0->hVal, c0->hGrad, c0->hm, seq, batch_ab(batch, 1, 1)) != 0)
          return false;                              // nothing was launched: no flags to wait for
      } else {
        launch_acq(st, &tab, c0->hXq, PCABO_INLAUNCH_MAXQ, gm, p, c0->dPartial, c0->dCounters, c0->dVal, c0->dGrad, c0->hVal,
                   c0->hGrad, c0->hm, seq, nullptr, nullptr, batch_ab(batch, 1, 1), B, n);
      }
      if (hipGetLastError() != hipSuccess) return false;
      const auto deadline = deadline_in(20);
      for (int e = 0; e < n; ++e) {
        const unsigned u = ent[e];
        const int q0 = groups ? (int)((u >> 8) & 0xffu) : (int)(u & 0xffffu), nq = groups ? (int)(u & 0xffu) : 1;
        if (wait_flags(batch->ctx[u >> 16]->hm, q0, nq, seq, deadline) != FLAGS_SET) return false;
      }
      return true;
    };
    auto stage = [&](int b, const RestartGroup& rg) {
      if (use_group) ent[nent++] = group_entry(b, rg.q0, rg.nq);
      else for (int j = 0; j < rg.nq; ++j) ent[nent++] = query_entry(b, rg.q0 + j);
    };
    const int rc = run_rounds(runs.data(), mine, stage, [&] { return launch(pg, use_group) ? PCABO_OK : PCABO_ERR_HIP; });
    for (int b : mine) if (runs[b].status == PCABO_ERR_NAN) set_err(batch->ctx[b], PCABO_ERR_NAN, "NaN in acquisition gradient%s", "");
    if (rc != PCABO_OK) { hip_failed.store(1); return; }
    // end points, values there (botorch evaluates once more at the clamped end points; normally that is the last point
    // the run evaluated - same kernel arithmetic, same bits - otherwise one value-only launch for the gang's leftovers)
    std::vector<int> redo;
    for (int b : mine) {
      RunRestarts& run = runs[b];
      if (run.status != PCABO_OK) continue;
      double* cb = cand + (size_t)b * num_restarts * MD;
      if (run.end_points(cb, vals + (size_t)b * num_restarts) == 0) continue;
      memcpy(run.xq, cb, (size_t)num_restarts * batch->ctx[b]->st.k * sizeof(double));
      for (int j = 0; j < num_restarts; ++j) ent[nent++] = query_entry(b, j);
      redo.push_back(b);
    }
    if (nent > 0) {
      if (!launch(pv, false)) { hip_failed.store(1); return; }
      for (int b : redo) std::copy(runs[b].val, runs[b].val + num_restarts, vals + (size_t)b * num_restarts);
    }
  };
  batch->pool.run(gang);
  if (hip_failed.load()) {
    batch->st.m.launch_may_have_died();
    (void)hipDeviceSynchronize();
    return bset_err(batch, PCABO_ERR_HIP, "an acquisition launch of the batch failed or did not answer%s", "");
  }
  for (int b = 0; b < B; ++b) {
    const bool any_failed = runs[b].report(info, (size_t)b * ngroups);
    if (failed) failed[b] = any_failed;
    if (status) status[b] = runs[b].status;
  }
  return PCABO_OK;
}

int pcabo_batch_optimize_acqf(pcabo_batch* batch, const double* ics, int num_restarts, int batch_limit,
                              const double* bounds, int maxiter, const double* best_f, int maximize, int acq,
                              double* cand, double* vals, int* info, int* failed, int* status) {
  if (!batch) return PCABO_ERR_ARG;
  if (!ics || !bounds || !best_f || !cand || !vals || num_restarts < 1 || batch_limit < 1 || num_restarts > PCABO_INLAUNCH_MAXQ)
    return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_optimize_acqf: bad argument (num_restarts <= 32)%s", "");
  if (const char* why = batch_acq_arg_error(batch, acq, best_f)) return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_optimize_acqf: %s", why);
  if (!batch->st.m.conditioned()) return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_optimize_acqf: no conditioned GP%s", "");
  // (the pinned point / value buffers and the runs' best_f words belong to an enqueued call until its _end)
  if (batch->st.opt_enqueued) return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_optimize_acqf: an optimisation of this batch is already enqueued%s", "");
  BHIPCHK(hipSetDevice(batch->device));
  if (const int rc = batch_put_best_f(batch, best_f)) return rc;
  batch->dbg_branches.clear(); batch->dbg_group_out.clear();      // (a call that takes the host-paced path leaves no debug record)
  std::vector<int> act;
  if (batch->dev_lbfgsb && device_opt_eligible(batch, num_restarts, batch_limit, bounds, maxiter, &act)) {
    if (batch->dev_lbfgsb == 2)
      return batch_optimize_twin(batch, act, ics, num_restarts, batch_limit, bounds, maxiter, maximize, acq, cand, vals, info, failed, status);
    const int rc = device_opt_enqueue(batch, act, ics, num_restarts, batch_limit, bounds, maxiter, maximize, acq);
    return rc != PCABO_OK ? rc : device_opt_collect(batch, num_restarts, batch_limit, cand, vals, info, failed, status);
  }
  return batch_optimize_host(batch, ics, num_restarts, batch_limit, bounds, maxiter, maximize, acq, cand, vals, info, failed, status);
}

// pcabo_batch_optimize_acqf in two halves for callers that drive several batches from one thread (PCABO_OPT_DEVICE_LBFGSB = 1
// only: the whole optimisation is one launch, so _begin returns as soon as it is enqueued).  _begin returns PCABO_OK, an error,
// or 1 when the call does not qualify for the device-resident optimiser - the caller then uses pcabo_batch_optimize_acqf.
int pcabo_batch_optimize_acqf_begin(pcabo_batch* batch, const double* ics, int num_restarts, int batch_limit,
                                    const double* bounds, int maxiter, const double* best_f, int maximize, int acq) {
  if (!batch) return PCABO_ERR_ARG;
  if (!ics || !bounds || !best_f || num_restarts < 1 || batch_limit < 1 || num_restarts > PCABO_INLAUNCH_MAXQ)
    return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_optimize_acqf_begin: bad argument (num_restarts <= 32)%s", "");
  if (const char* why = batch_acq_arg_error(batch, acq, best_f)) return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_optimize_acqf_begin: %s", why);
  if (!batch->st.m.conditioned()) return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_optimize_acqf_begin: no conditioned GP%s", "");
  if (batch->st.opt_enqueued) return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_optimize_acqf: an optimisation of this batch is already enqueued%s", "");
  if (batch->dev_lbfgsb != 1) return 1;
  BHIPCHK(hipSetDevice(batch->device));
  if (const int rc = batch_put_best_f(batch, best_f)) return rc;
  std::vector<int> act;
  if (!device_opt_eligible(batch, num_restarts, batch_limit, bounds, maxiter, &act)) return 1;
  return device_opt_enqueue(batch, act, ics, num_restarts, batch_limit, bounds, maxiter, maximize, acq);
}
int pcabo_batch_optimize_acqf_end(pcabo_batch* batch, int num_restarts, int batch_limit, double* cand, double* vals, int* info,
                                  int* failed, int* status) {
  if (!batch || !cand || !vals) return PCABO_ERR_ARG;
  BHIPCHK(hipSetDevice(batch->device));
  return device_opt_collect(batch, num_restarts, batch_limit, cand, vals, info, failed, status);
}

// Value and gradient of the acquisition at q <= 32 points per run through the evaluation of the device-resident optimiser
// (mode 0 of k_lbfgsb_group; PCABO_OPT_DEVICE_LBFGSB must be on so that the transposed root inverse exists).  Xq[B][q * max_d]
// (run b's points packed with stride k_b), val[B][q], grad[B][q * max_d] (same packing).  Diagnostics / parity tests.
int pcabo_batch_device_acq_eval(pcabo_batch* batch, const double* Xq, int q, const double* best_f, int maximize, int acq,
                                double* val, double* grad) {
  if (!batch) return PCABO_ERR_ARG;
  if (!Xq || !best_f || !val || !grad || q < 1 || q > PCABO_INLAUNCH_MAXQ)
    return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_device_acq_eval: bad argument (q <= 32)%s", "");
  if (const char* why = batch_acq_arg_error(batch, acq, best_f)) return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_device_acq_eval: %s", why);
  if (!batch->st.m.conditioned() || !batch->dev_lbfgsb)
    return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_device_acq_eval: needs a conditioned GP and PCABO_OPT_DEVICE_LBFGSB%s", "");
  // the pinned table / point / value / gradient buffers below belong to an enqueued call until its _end has collected them
  if (batch->st.begin_pending())
    return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_device_acq_eval: a _begin call of this batch has not been ended%s", "");
  BHIPCHK(hipSetDevice(batch->device));
  const int MD = batch->max_d;
  if (!lbfgsb_device_possible(batch->st.m.NP, batch_max_k(batch), PCABO_GROUP_Q) || !opt_fits(batch->ctx[0]->lay, q, 0, batch_max_k(batch)))
    return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_device_acq_eval: shape beyond the device optimiser (n <= 512, k <= 40)%s", "");
  if (const int rc = batch_put_best_f(batch, best_f)) return rc;
  std::vector<int> runs;
  for (int b = 0; b < batch->B; ++b) if (batch->ctx[b]->st.conditioned()) runs.push_back(b);
  int nent = 0;
  for (int b : runs) {
    pcabo_ctx* c = batch->ctx[b];
    memcpy(c->hXq, Xq + (size_t)b * q * MD, (size_t)q * c->st.k * sizeof(double));
    for (int q0 = 0; q0 < q; q0 += PCABO_GROUP_Q)
      batch->hOptTab[nent++] = group_entry(b, q0, std::min(PCABO_GROUP_Q, q - q0));
  }
  if (nent == 0) return PCABO_OK;
  if (const int rc = device_opt_launch(batch, nent, 0, q, PCABO_GROUP_Q, 1, maximize, acq, val_opt_values(q))) return rc;
  BHIPCHK(wait_stream(batch->stream));
  BHIPCHK(hipGetLastError());
  for (int b : runs) {
    const pcabo_ctx* c = batch->ctx[b];
    memcpy(val + (size_t)b * q, c->hVal, (size_t)q * sizeof(double));
    memcpy(grad + (size_t)b * q * MD, c->hGrad, (size_t)q * c->st.k * sizeof(double));
  }
  return PCABO_OK;
}

// the inverse map of every run's candidate in two halves (x_ok: the caller's x is there - asked before anything is written)
static int batch_inverse_map_enqueue(pcabo_batch* batch, const double* z, bool x_ok = true) {
  if (!batch || !z || !x_ok) return PCABO_ERR_ARG;
  if (!batch->st.wpca_on_host()) return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_inverse_map: no weighted PCA collected%s", "");
  BHIPCHK(hipSetDevice(batch->device));
  hipStream_t s = batch->stream;
  pcabo_ctx* c0 = batch->ctx[0];
  const int B = batch->B, MD = batch->max_d, d = batch->st.m.d;
  for (int b = 0; b < B; ++b) memcpy(batch->ctx[b]->hXq, z + (size_t)b * MD, (size_t)batch->ctx[b]->st.k * sizeof(double));
  BHIPCHK(hipMemcpy2DAsync(c0->dZq, batch->zs, c0->hXq, batch->hzs, (size_t)MD * sizeof(double), B, hipMemcpyHostToDevice, s));
  launch_inverse_map(s, c0->dZq, c0->dComps, c0->dDataMean, c0->dPcaMean, 0, d, c0->dXout, c0->dK, batch_zb(batch));
  BHIPCHK(hipMemcpy2DAsync(small_at(c0, small_imap_x(c0->lay.s)), batch->hzs, c0->dXout, batch->zs, (size_t)d * sizeof(double), B, hipMemcpyDeviceToHost, s));
  BHIPCHK(hipGetLastError());
  batch->st.imap_begun();
  return PCABO_OK;
}
static int batch_inverse_map_collect(pcabo_batch* batch, double* x) {
  if (!batch || !x) return PCABO_ERR_ARG;
  if (!batch->st.imap_enqueued) return bset_err(batch, PCABO_ERR_ARG, "pcabo_batch_inverse_map_end: no _begin before it%s", "");
  BHIPCHK(hipSetDevice(batch->device));
  batch->st.imap_ended();
  BHIPCHK(wait_stream(batch->stream));
  BHIPCHK(hipGetLastError());
  const int d = batch->st.m.d;
  for (int b = 0; b < batch->B; ++b) memcpy(x + (size_t)b * d, small_at(batch->ctx[b], small_imap_x(batch->ctx[b]->lay.s)), (size_t)d * sizeof(double));
  return PCABO_OK;
}
int pcabo_batch_inverse_map(pcabo_batch* batch, const double* z, double* x) {
  const int rc = batch_inverse_map_enqueue(batch, z, x != nullptr);
  return rc != PCABO_OK ? rc : batch_inverse_map_collect(batch, x);
}
int pcabo_batch_inverse_map_begin(pcabo_batch* batch, const double* z) { return batch_inverse_map_enqueue(batch, z); }
int pcabo_batch_inverse_map_end(pcabo_batch* batch, double* x) { return batch_inverse_map_collect(batch, x); }

}  // extern "C"

// =====================================================================================================================
// Final gather of best-so-far values over RCCL (declared in include/pcabo.h).
// The data path has no collective: runs are independent and every rank drives its own GPU.  The ONE exchange of the design -
// the all-gather of a few doubles after the runs - is available here for callers without torch.distributed.  librccl.so is
// opened on first use (no link-time dependency: a process that never gathers never loads it).
// =====================================================================================================================
#include <dlfcn.h>

namespace {
typedef struct { char internal[128]; } rccl_unique_id;            // ncclUniqueId (NCCL_UNIQUE_ID_BYTES = 128)
struct RcclApi {
  void* lib = nullptr;
  int (*GetUniqueId)(rccl_unique_id*) = nullptr;
  int (*CommInitRank)(void**, int, rccl_unique_id, int) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  bool ok = false;
};
RcclApi& rccl() {
  static RcclApi api = [] {
    RcclApi a;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      a.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (a.lib) break;
    }
    if (!a.lib) return a;
    a.GetUniqueId = (int (*)(rccl_unique_id*))dlsym(a.lib, "ncclGetUniqueId");
    a.CommInitRank = (int (*)(void**, int, rccl_unique_id, int))dlsym(a.lib, "ncclCommInitRank");
    a.AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(a.lib, "ncclAllGather");
    a.CommDestroy = (int (*)(void*))dlsym(a.lib, "ncclCommDestroy");
    a.GetErrorString = (const char* (*)(int))dlsym(a.lib, "ncclGetErrorString");
    a.ok = a.GetUniqueId && a.CommInitRank && a.AllGather && a.CommDestroy;
    return a;
  }();
  return api;
}
}  // namespace

struct pcabo_comm {
  void* comm = nullptr;
  int world = 0, rank = 0, device = 0;
  hipStream_t stream = nullptr;
  double* dbuf = nullptr;
  size_t cap = 0;                       // doubles per rank the device buffer holds
  char err[256] = {0};
};
static int cset_err(pcabo_comm* c, int code, const char* what, int rc) {
  if (c) {
    const RcclApi& a = rccl();
    snprintf(c->err, sizeof(c->err), "%s (%d%s%s)", what, rc, a.GetErrorString ? ": " : "", a.GetErrorString ? a.GetErrorString(rc) : "");
  }
  return code;
}

extern "C" {

int pcabo_comm_unique_id(char* id128) {
  if (!id128) return PCABO_ERR_ARG;
  RcclApi& a = rccl();
  if (!a.ok) return PCABO_ERR_HIP;
  rccl_unique_id id;
  if (a.GetUniqueId(&id) != 0) return PCABO_ERR_HIP;
  memcpy(id128, id.internal, 128);
  return PCABO_OK;
}

int pcabo_comm_create(const char* id128, int world, int rank, int device, pcabo_comm** out) {
  if (!out) return PCABO_ERR_ARG;
  *out = nullptr;
  if (!id128 || world < 1 || rank < 0 || rank >= world) return PCABO_ERR_ARG;
  RcclApi& a = rccl();
  if (!a.ok) return PCABO_ERR_HIP;
  pcabo_comm* c = new (std::nothrow) pcabo_comm();
  if (!c) return PCABO_ERR_HIP;
  *out = c;                             // handed back even on failure (message in pcabo_comm_last_error)
  c->world = world; c->rank = rank; c->device = device;
  if (hipSetDevice(device) != hipSuccess) return cset_err(c, PCABO_ERR_HIP, "hipSetDevice failed", (int)hipGetLastError());
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return cset_err(c, PCABO_ERR_HIP, "stream", (int)hipGetLastError());
  rccl_unique_id id;
  memcpy(id.internal, id128, 128);
  const int rc = a.CommInitRank(&c->comm, world, id, rank);
  if (rc != 0) { c->comm = nullptr; return cset_err(c, PCABO_ERR_HIP, "ncclCommInitRank failed", rc); }
  return PCABO_OK;
}

int pcabo_gather_best(pcabo_comm* c, const double* local, int n_local, double* all) {
  if (!c || !c->comm || !local || !all || n_local < 1) return PCABO_ERR_ARG;
  RcclApi& a = rccl();
  if (hipSetDevice(c->device) != hipSuccess) return cset_err(c, PCABO_ERR_HIP, "hipSetDevice failed", (int)hipGetLastError());
  if ((size_t)n_local > c->cap) {
    if (c->dbuf) (void)hipFree(c->dbuf);
    c->dbuf = nullptr; c->cap = 0;
    if (hipMalloc((void**)&c->dbuf, (size_t)n_local * (c->world + 1) * sizeof(double)) != hipSuccess)
      return cset_err(c, PCABO_ERR_HIP, "hipMalloc failed", (int)hipGetLastError());
    c->cap = (size_t)n_local;
  }
  double* send = c->dbuf;
  double* recv = c->dbuf + c->cap;
  if (hipMemcpyAsync(send, local, (size_t)n_local * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess)
    return cset_err(c, PCABO_ERR_HIP, "copy to the device failed", (int)hipGetLastError());
  const int rc = a.AllGather(send, recv, (size_t)n_local, /* ncclFloat64 */ 8, c->comm, c->stream);
  if (rc != 0) return cset_err(c, PCABO_ERR_HIP, "ncclAllGather failed", rc);
  if (hipMemcpyAsync(all, recv, (size_t)n_local * c->world * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess)
    return cset_err(c, PCABO_ERR_HIP, "copy from the device failed", (int)hipGetLastError());
  return PCABO_OK;
}

int pcabo_comm_last_error(pcabo_comm* c, char* buf, int buflen) {
  if (!c || !buf || buflen <= 0) return PCABO_ERR_ARG;
  snprintf(buf, buflen, "%s", c->err);
  return PCABO_OK;
}

int pcabo_comm_destroy(pcabo_comm* c) {
  if (!c) return PCABO_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->comm) (void)rccl().CommDestroy(c->comm);
  if (c->dbuf) (void)hipFree(c->dbuf);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return PCABO_OK;
}

}  // extern "C"
