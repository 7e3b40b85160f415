// Engine: device memory, step plan, HIP graphs, voice and slot management.
//
// Data layout in HBM (fp32):
//   weight blob                packed by weights.cpp (one allocation; RCCL-broadcastable)
//   FlowLM KV                  [slot][layer][k|v][head][max_ctx][64]   (attention.rs:211-231, preallocated;
//                              positions < F of an admitted slot are read from its voice's own
//                              [layer][k|v][head][F][64] cache, shared by every slot of that voice)
//   Mimi KV ring               [slot][layer][k|v][head][512][64]       (attention.rs:167-264, ctx 250)
//   conv histories             [slot][P][C] per streaming conv          (conv.rs:71-136, time-major)
//   activations                row-major [rows][features]; Mimi/SEANet channels-last [slot][time][ch]
#include "engine.h"

#include <hip/hip_ext.h>

#include <algorithm>
#include <array>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <mutex>

namespace ptts {

namespace {
// voice reference counts (ptts_voice::refs / dead): engines and ptts_voice_destroy may run on
// different host threads
std::mutex& voice_mu() {
  static std::mutex m;
  return m;
}

int pick_splits(int M, int N, int K) {
  const int tiles = ((N + 31) / 32) * ((M + 31) / 32);
  const int chunks = K / 32;
  int s = std::max(1, 768 / std::max(1, tiles));
  s = std::min(s, std::max(1, chunks / 4));
  return std::min(s, 16);  // k_row_reduce sums at most 16 slabs
}
}  // namespace

// Tuning override of an op's tile layout / split-K count (tools/back_tune.py, probe builds only):
// PTTS_OVR="name=L[:S],...", read at every plan build.
static void tile_override(const std::string& name, int& layout, int& ksplit) {
  const char* e = probe_env("PTTS_OVR");
  if (!e) return;
  const std::string s(e);
  size_t p = 0;
  while (p < s.size()) {
    size_t q = s.find(',', p);
    if (q == std::string::npos) q = s.size();
    const std::string item = s.substr(p, q - p);
    p = q + 1;
    const size_t eq = item.find('=');
    if (eq == std::string::npos || item.compare(0, eq, name) != 0 || eq != name.size()) continue;
    const std::string v = item.substr(eq + 1);
    const size_t c = v.find(':');
    layout = atoi(v.substr(0, c).c_str());
    if (c != std::string::npos) ksplit = atoi(v.substr(c + 1).c_str());
  }
}

// The row of a tile id in this build's table (kernels.h PTTS_TILES)
static const TileInfo& tile_of(int layout) {
  const TileInfo* t = tile_info(layout);
  if (!t) throw Error(PTTS_ERR_INVALID, "gemm: tile layout " + std::to_string(layout) + " is not in this build");
  return *t;
}

float* Engine::dalloc(size_t n) {
  void* p = nullptr;
  PTTS_HIP(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(float)));
  PTTS_HIP(hipMemset(p, 0, std::max<size_t>(n, 1) * sizeof(float)));
  // hipMemset runs on the null stream, which does not order against the engine's non-blocking
  // streams: wait for it, or a kernel that fills the buffer next on stream_ can be overwritten
  // by the zeroing (seen: the transposed input-projection weight zeroed under quantized engines)
  PTTS_HIP(hipDeviceSynchronize());
  allocs_.push_back(p);
  return (float*)p;
}

// dalloc's pinned-host counterpart (not zeroed): freed by the destructor's one loop
void* Engine::halloc(size_t bytes) {
  void* p = nullptr;
  PTTS_HIP(hipHostMalloc(&p, bytes, hipHostMallocDefault));
  hallocs_.push_back(p);
  return p;
}

// The back part's workspace and codec state for `rows` rows and passes of up to nfr frames, all zero:
// the fresh state every utterance starts from
Engine::BackBufs Engine::back_alloc(int rows, int nfr) {
  const size_t P = (size_t)rows, BF = P * nfr;  // utterance frames of one pass
  BackBufs b;
  b.ring = dalloc((size_t)ring_slot_ * P);
  b.mpos = (int*)dalloc(P);
  // overlap-add history [row][512] (the last committed frame's quantizer output) and the
  // pass's quantizer outputs [row][NFR_MAX][512], copied into it by the commit (quant_upsample)
  b.qprev = dalloc((size_t)(1 + NFR_MAX) * P * MD);
  b.qcur = b.qprev + P * MD;
  b.mx = dalloc(BF * UP * MD);
  b.mh = dalloc(BF * UP * MD);
  b.mq = dalloc(BF * UP * MD);
  b.mo = dalloc(BF * UP * MD);
  b.mqkv = dalloc(BF * UP * 3 * MD);
  b.mu = dalloc(BF * UP * MFF);
  b.a0 = dalloc(BF * 16 * 512);
  int T = 16, ch = 512;
  for (int i = 0; i < 3; ++i) {
    T *= RATIOS[i];
    ch /= 2;
    b.cb[i] = dalloc(BF * T * ch);
    b.ce[i] = dalloc(BF * T * ch);
    b.cv[i] = dalloc(BF * T * (ch / 2));
    b.ca[i] = dalloc(BF * T * ch);
  }
  // split-K slabs: up to 8 slices of the Mimi / conv0 rows (rows * 16 x 512), 4 of the stage-0
  // transposed conv (rows * 16 x 6 * 256), per frame of a pass
  b.mpcap = (size_t)nfr * std::max({(size_t)8 * P * UP * MD, (size_t)4 * P * UP * RATIOS[0] * (MD / 2)});
  b.mpartial = dalloc(b.mpcap);
  for (int i = 0; i < 8; ++i) b.hist[i] = dalloc(P * hist_P_[i] * hist_C_[i]);
  b.fin_side = dalloc(P * (nfr * FRAME / RESBLOCK_FIN_TT) * 2);
  return b;
}

Engine::Engine(const ptts_engine_config& cfg) {
  check_model_config(cfg.cfg_yaml);  // before any device work
  PTTS_REQUIRE(cfg.max_slots >= 1 && cfg.max_slots <= 256, "max_slots must be in [1, 256]");
  PTTS_REQUIRE(cfg.max_ctx >= 16 && cfg.max_ctx <= 8192, "max_ctx must be in [16, 8192]");
  PTTS_REQUIRE(cfg.lsd_decode_steps >= 1 && cfg.lsd_decode_steps <= LSD_MAX, "lsd_decode_steps must be in [1, 64]");
  dev_ = cfg.device;
  max_slots_ = cfg.max_slots;
  max_ctx_ = cfg.max_ctx;
  lsd_ = cfg.lsd_decode_steps;
  PTTS_REQUIRE(cfg.weight_quant >= QUANT_NONE && cfg.weight_quant <= QUANT_ALL, "unknown weight_quant mode");
  wq_ = cfg.weight_quant;
  PTTS_REQUIRE(cfg.fp8_gemm == 0 || cfg.fp8_gemm == 1, "fp8_gemm must be 0 or 1");
  PTTS_REQUIRE(!(cfg.fp8_gemm && cfg.weight_quant != QUANT_NONE), "fp8_gemm and weight_quant are exclusive");
  fp8_ = cfg.fp8_gemm;
  PTTS_REQUIRE(cfg.back_frames >= 0 && cfg.back_frames <= NFR_MAX && !(cfg.back_frames & (cfg.back_frames - 1)),
               "back_frames must be 0, 1, 2, 4 or 8");
  nfr_ = cfg.pipeline && cfg.back_frames >= 2 ? cfg.back_frames : 1;
  PTTS_REQUIRE(cfg.back_mfma >= PTTS_BACK_F32 && cfg.back_mfma <= PTTS_BACK_F32X6, "unknown back_mfma mode");
  back_mfma_ = cfg.back_mfma;
  nhb_ = nfr_ > 1 ? 3 * nfr_ : 3;
  int ndev = 0;
  PTTS_HIP(hipGetDeviceCount(&ndev));
  PTTS_REQUIRE(dev_ >= 0 && dev_ < ndev, "HIP device ordinal out of range");
  PTTS_HIP(hipSetDevice(dev_));
  PTTS_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));

  L_ = pack_weights(nullptr, nullptr);
  if (cfg.weight_blob) {
    blob_ = (float*)cfg.weight_blob;
    own_blob_ = false;
  } else {
    blob_ = dalloc(L_.total);
  }

  const int B = max_slots_;
  fbm_.kv_layer = (long)2 * NH * max_ctx_ * 64;
  fbm_.kv = KvStore{dalloc((size_t)fbm_.kv_layer * NL * B), fbm_.kv_layer * NL, max_ctx_};
  ring_layer_ = (long)2 * MNH * RING * 64;
  ring_slot_ = ring_layer_ * MNL;
  // streaming conv histories (SEANetDecoder, seanet.rs:307-402): source T, channels, rows kept
  const int hT[8] = {16, 16, 96, 96, 480, 480, 1920, 1920};
  const int hC[8] = {512, 512, 256, 256, 128, 128, 64, 64};
  const int hP[8] = {6, 1, 2, 1, 2, 1, 2, 2};
  for (int i = 0; i < 8; ++i) hist_T_[i] = hT[i], hist_C_[i] = hC[i], hist_P_[i] = hP[i];
  bbm_ = back_alloc(B, nfr_);
  fpos_ = (int*)dalloc(B);
  st_ = (SlotState*)dalloc((sizeof(SlotState) * B + 3) / 4);
  lat_in_ = dalloc((size_t)B * LDIM);
  cur_ = dalloc((size_t)B * LDIM);
  eos_ = dalloc(B);
  static_assert(sizeof(FrameFlags) == 2 * sizeof(float), "FrameFlags packs into two floats");
  meta_floats_ = (size_t)B * (LDIM + 1 + 2);
  // multi-frame passes: pass p's PCM [B][nfr][1920] and the meta blocks of its buffers nfr p ..
  // nfr p + nfr - 1 in ONE device block and ONE pinned host block, so the pass delivers its frames
  // with one copy node (a 128-B multiple per meta block keeps FrameFlags 8-B aligned)
  const size_t mstride = (meta_floats_ + 31) / 32 * 32;
  if (nfr_ > 1)
    for (int p = 0; p < nhb_ / nfr_; ++p) {
      const size_t n = (size_t)B * nfr_ * FRAME + nfr_ * mstride;
      pcmp_[p] = dalloc(n);
      h_pcmp_[p] = (float*)halloc(sizeof(float) * n);
    }
  for (int q = 0; q < NHB; ++q) {  // front -> back hand-off buffers
    meta_[q] = nfr_ > 1 && q < nhb_ ? pcmp_[q / nfr_] + (size_t)B * nfr_ * FRAME + (q % nfr_) * mstride
                                    : dalloc(meta_floats_);
    lat_out_[q] = meta_[q];                                  // 128-B aligned,
    flags_[q] = (FrameFlags*)(meta_[q] + (size_t)B * LDIM);  // so FrameFlags stay 8-B aligned
    eos_out_[q] = meta_[q] + (size_t)B * (LDIM + 2);
    pcm_[q] = dalloc((size_t)B * FRAME);
  }
  h_act_ = (SlotState*)halloc(sizeof(SlotState) * B);

  const int R = std::max(B, PREFILL);
  fbm_.x = dalloc((size_t)R * D);
  fbm_.h = dalloc((size_t)R * D);
  fbm_.q = dalloc((size_t)R * D);
  fbm_.o = dalloc((size_t)R * D);
  fbm_.u = dalloc((size_t)R * FF);
  // split-K slabs: skinny FlowLM/head GEMMs, and the 2-way split Mimi QKV (B*16 rows x 1536)
  fbm_.pcap = std::max({(size_t)4 << 20, (size_t)2 * B * UP * 3 * MD, (size_t)PREFILL * FF});
  fbm_.partial = dalloc(fbm_.pcap);
  fbm_.tslab = dalloc(TAIL_CAP);
  fbm_.tail_cap = (long)TAIL_CAP;
  fbm_.tickets = (int*)dalloc(TICKETS);  // zero; every split-tail launch leaves them zero
  ids_dev_ = (int*)dalloc(PREFILL);
  rowtab_dev_ = (int*)dalloc(PREFILL);
  ctab_dev_ = (int*)dalloc(PREFILL);
  qrow_dev_ = (int*)dalloc(PREFILL);
  orow_dev_ = (int*)dalloc(PREFILL);
  admit_slots_ = (int*)dalloc(B);
  admit_st_ = (SlotState*)dalloc((sizeof(SlotState) * B + 3) / 4);
  admit_fpos_ = (int*)dalloc(B);
  plat_dev_ = dalloc((size_t)PREFILL * LDIM);
  admit_lat_ = dalloc((size_t)B * LDIM);
  admit_opt_ = (int*)dalloc(B);
  vpre_ = (const float**)dalloc((sizeof(float*) * B + 3) / 4);  // zero: no slot has a prefix
  vlen_ = (int*)dalloc(B);
  slot_voice_.assign(B, nullptr);
  drained_.assign(B, 1);
  codec_ok_.assign(B, 1);
  admit_call_.assign(B, -1);
  slot_lsd_.assign(B, 0);
  cancelled_.assign(B, 0);
  share_voice_ = probe_env("PTTS_NO_SHARED_VOICE") == nullptr;
  if (share_voice_) {  // positions below a slot's voice length read the voice's own cache
    fbm_.kv.pre = vpre_;
    fbm_.kv.pre_len = vlen_;
  }
#ifdef PTTS_PROBES
  if (probe_env("PTTS_STAMPS")) {
    stamp_ring_ = (unsigned long long*)dalloc((size_t)STAMP_CAP * 4);
    stamp_ctr_ = (unsigned*)dalloc(1);
  }
#endif
  // pipelined stepping: the back part's kernels run at most one workgroup per CU, so the
  // latency-bound front part always finds room on every CU (measured 0.735 -> 0.688 ms per step
  // for the GEMMs alone; tools/sweep_env.sh)
  // three hand-off buffers: the front part may run two frames ahead of the back part. With the
  // back part now the longer of the two alone (498 vs 441 us), the front no longer idles behind
  // it: steady step 0.6370 -> 0.6321 ms (medians of 4; when the front was the longer part, 3
  // buffers measured 0.5% slower).
  if (probe_env("PTTS_BACK_WG_CAP")) back_cap_ = atoi(probe_env("PTTS_BACK_WG_CAP"));
  if (probe_env("PTTS_FRONT_PRIO")) set_front_prio(atoi(probe_env("PTTS_FRONT_PRIO")));
  if (probe_env("PTTS_BACK_PRIO")) set_back_prio(atoi(probe_env("PTTS_BACK_PRIO")));
  if (probe_env("PTTS_FRONT_SKIP")) set_front_skip(atoi(probe_env("PTTS_FRONT_SKIP")));
  ysilu_ = dalloc((size_t)lsd_ * B * FD);
  mods_ = dalloc((size_t)lsd_ * B * NADA);
  xf_ = dalloc((size_t)B * FD);
  hf_ = dalloc((size_t)B * FD);
  uf_ = dalloc((size_t)B * FD);
  PTTS_REQUIRE(hx_floats(B) * 4 < (1ull << 31), "flow-head hand-off regions exceed 2 GB (lsd_decode_steps too large)");
  hx_ = dalloc(hx_floats(B));
  // adaLN shift / scale in the chain's fragment order (written by the adaLN reduce), zeroed:
  // rows past B in the last row group read finite values and are never stored
  fhm_ = dalloc((size_t)lsd_ * ((B + 15) / 16) * (FDEPTH + 1) * 2 * 16 * FD);
  PTTS_HIP(hipMemset(hx_, 0xFF, hx_floats(B) * 4));  // empty (the launch ahead re-arms the used part)
  PTTS_HIP(hipDeviceSynchronize());                    // null-stream memset: see dalloc
  hp_hand_ = dalloc((size_t)lsd_ * 2 * HP_REGION_FLOATS);
  hctr_ = (int*)dalloc(4 * ((B + 15) / 16) + 4);
  herr_ = (int*)dalloc(4);
  for (int i = 0, ch = MD / 2; i < 3; ++i, ch /= 2) trb_[i] = dalloc((size_t)RATIOS[i] * ch);
  temb_ =dalloc((size_t)temb_row0(lsd_ + 1) * FD);  // every count 1 .. lsd_, triangular (finalize)
  rope_ = dalloc((size_t)max_ctx_ * 64);
  temb_tmp_ = dalloc((size_t)2 * lsd_ * FD);

  for (int q = 0; q < NHB; ++q) {
    h_pcm_[q] = (float*)halloc(sizeof(float) * B * FRAME);
    // inside the pass's pinned block (above), or a block of its own
    h_meta_[q] = nfr_ > 1 && q < nhb_ ? h_pcmp_[q / nfr_] + (size_t)B * nfr_ * FRAME + (q % nfr_) * mstride
                                      : (float*)halloc(sizeof(float) * meta_floats_);
    memset(h_meta_[q], 0, sizeof(float) * meta_floats_);
  }
  h_err_ = (int*)halloc(sizeof(int));
  *h_err_ = 0;
  h_slots_ = (int*)halloc(sizeof(int) * B);
  h_st_ = (SlotState*)halloc(sizeof(SlotState) * B);
  h_idle_ = (SlotState*)halloc(sizeof(SlotState));
  *h_idle_ = SlotState{};
  h_idle_->eos_step = -1;
  h_fp_ = (int*)halloc(sizeof(int) * B);
  h_ids_ = (int*)halloc(sizeof(int) * PREFILL);
  h_tab_ = (int*)halloc(sizeof(int) * 4 * PREFILL);  // ptab | ctab | qrow | orow
  h_plat_ = (float*)halloc(sizeof(float) * PREFILL * LDIM);
  h_alat_ = (float*)halloc(sizeof(float) * B * LDIM);
  h_aopt_ = (int*)halloc(sizeof(int) * B);
  h_vpre_ = (const float**)halloc(sizeof(const float*) * B);
  h_vlen_ = (int*)halloc(sizeof(int) * B);
  memset(h_vpre_, 0, sizeof(float*) * B);
  memset(h_vlen_, 0, sizeof(int) * B);
  PTTS_HIP(hipStreamCreateWithFlags(&stream_be_, hipStreamNonBlocking));
  for (int q = 0; q < NHB; ++q) {
    PTTS_HIP(hipEventCreateWithFlags(&ev_front_[q], hipEventDisableTiming));
    PTTS_HIP(hipEventCreateWithFlags(&ev_back_[q], hipEventDisableTiming));
    PTTS_HIP(hipEventRecord(ev_front_[q], stream_));
    PTTS_HIP(hipEventRecord(ev_back_[q], stream_));
  }
  PTTS_HIP(hipEventCreateWithFlags(&ev_admit_, hipEventDisableTiming));
  PTTS_HIP(hipEventCreateWithFlags(&ev_be_tail_, hipEventDisableTiming));
  PTTS_HIP(hipEventCreateWithFlags(&ev_act_, hipEventDisableTiming));
  for (hipEvent_t& e : ev_call_) PTTS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  PTTS_HIP(hipEventRecord(ev_act_, stream_));
  PTTS_HIP(hipEventRecord(ev_admit_, stream_));
  pipeline_ = cfg.pipeline != 0;
  head_resident_ = flow_head_max_resident(dev_);

  if (!cfg.defer_weights) {
    std::unique_ptr<TensorSource> src = cfg.weights_path && cfg.weights_path[0]
                                            ? make_safetensors_source(cfg.weights_path)
                                            : make_synth_source(cfg.synth_seed);
    src = make_quant_source(std::move(src), wq_);
    upload_weights(src.get());
    finalize();
  }
}

Engine::~Engine() {
  (void)hipSetDevice(dev_);
  if (stream_) (void)hipStreamSynchronize(stream_);
  if (stream_be_) (void)hipStreamSynchronize(stream_be_);
  if (stream_pv_) (void)hipStreamSynchronize(stream_pv_);
  if (stream_vc_) (void)hipStreamSynchronize(stream_vc_);  // pending voice jobs write their voices
#ifdef PTTS_PROBES
  if (stamp_ring_) {  // tag (part << 8 | buffer << 1 | end), then the 100-MHz realtime count
    unsigned n = 0;
    std::vector<unsigned long long> r((size_t)STAMP_CAP * 2);
    if (hipMemcpy(&n, stamp_ctr_, 4, hipMemcpyDeviceToHost) == hipSuccess &&
        hipMemcpy(r.data(), stamp_ring_, r.size() * 8, hipMemcpyDeviceToHost) == hipSuccess)
      if (FILE* f = fopen(probe_env("PTTS_STAMPS"), "w")) {
        for (int p = 0; p < 2; ++p)
          for (size_t i = 0; i < stamp_names_[p].size(); ++i) fprintf(f, "# %d %zu %s\n", p, i, stamp_names_[p][i].c_str());
        for (unsigned i = 0; i < std::min(n, STAMP_CAP); ++i) fprintf(f, "%llu %llu\n", r[2 * i], r[2 * i + 1]);
        fclose(f);
      }
  }
#endif
  for (int s = 0; s < (int)slot_voice_.size(); ++s) voice_release(s, true);
  for (auto& kv : graphs_) (void)hipGraphExecDestroy(kv.second);
  for (auto& kv : graph_defs_) (void)hipGraphDestroy(kv.second);
  for (auto& kv : pv_graphs_) (void)hipGraphExecDestroy(kv.second);
  for (auto& kv : pv_graph_defs_) (void)hipGraphDestroy(kv.second);
  for (PvEntry& q : pv_q_)
    if (q.ev) (void)hipEventDestroy(q.ev);
  for (int q = 0; q < NHB; ++q)
    if (ev_pv_read_[q]) (void)hipEventDestroy(ev_pv_read_[q]);
  if (ev_pv_front_) (void)hipEventDestroy(ev_pv_front_);
  if (stream_pv_) (void)hipStreamDestroy(stream_pv_);
  for (int q = 0; q < NHB; ++q) {
    if (ev_front_[q]) (void)hipEventDestroy(ev_front_[q]);
    if (ev_back_[q]) (void)hipEventDestroy(ev_back_[q]);
  }
  if (ev_admit_) (void)hipEventDestroy(ev_admit_);
  if (ev_be_tail_) (void)hipEventDestroy(ev_be_tail_);
  if (ev_act_) (void)hipEventDestroy(ev_act_);
  for (hipEvent_t e : ev_call_)
    if (e) (void)hipEventDestroy(e);
  if (stream_be_) (void)hipStreamDestroy(stream_be_);
  vws_free(vws_);
  for (hipEvent_t e : vws_.ev_up)
    if (e) (void)hipEventDestroy(e);
  if (stream_vc_) (void)hipStreamDestroy(stream_vc_);
  for (void* p : allocs_) (void)hipFree(p);
  for (void* p : hallocs_) (void)hipHostFree(p);
  if (stream_) (void)hipStreamDestroy(stream_);
}

void Engine::upload_weights(TensorSource* src) {
  std::vector<float> host(L_.total, 0.f);
  pack_weights(src, host.data());
  PTTS_HIP(hipMemcpy(blob_, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
}

void Engine::load_blob(const float* host, size_t n_bytes) {
  PTTS_REQUIRE(n_bytes == L_.total * sizeof(float), "blob size differs from ptts_weight_blob_bytes()");
  PTTS_REQUIRE(!ready_, "engine already finalized");
  PTTS_HIP(hipSetDevice(dev_));
  PTTS_HIP(hipMemcpy(blob_, host, n_bytes, hipMemcpyHostToDevice));
}

// The FlowLM step matrices as fragment-packed copies for the register-resident split-K GEMM
// (bit mask of the matrices that use it: 1 qkv, 2 out, 4 linear1, 8 linear2, 16 the flow head's
// adaLN matrix, M = lsd * B rows): out on 32x32 tiles with 8 K slices of 128 (4 waves splitting
// each), linear2 on 32x32 tiles with 16 slices of 256. Alone on the chip every matrix is faster
// this way (qkv 8.1 -> 4.9 us, out 4.5 -> 3.2, linear1 8.1 -> 5.2, linear2 7.9 -> 5.3); in the
// pipelined step only out + linear2 + adaLN pay (steady step 0.6595 -> 0.6326 ms, medians of 3):
// the qkv / linear1 versions on any tile slow the concurrent back part more than they gain.
// The int8 codes of quantized weight W [N][K] (derive_int8) in pack_q8 order: the codes widened
// to f32 (temporary), fragment-packed by `pack` exactly as the f32 weight would be, then one byte
// per element with a lane's four fragment groups per 16-B load (nj: groups per lane and wave).
// fp8_gemm engines: the e4m3 codes of fp8_codes (f8map_) the same way.
const uint32_t* Engine::pack_codes(const float* W, int N, int K, int nj,
                                   const std::function<void(const float*, float*)>& pack) {
  auto it = q8map_.find(W);
  auto it8 = f8map_.find(W);
  if (it == q8map_.end() && it8 == f8map_.end()) return nullptr;
  const size_t n = (size_t)N * K;
  float* tmp = nullptr;
  PTTS_HIP(hipMalloc(&tmp, sizeof(float) * 2 * n));
  void* q = nullptr;
  PTTS_HIP(hipMalloc(&q, n));
  allocs_.push_back(q);
  if (it != q8map_.end()) codes_to_f32(it->second.first, (long)n, tmp, stream_);
  else codes_u8_to_f32(it8->second.first, (long)n, tmp, stream_);
  pack(tmp, tmp + n);
  pack_q8(tmp + n, (long)(n / 4), nj, (uint32_t*)q, stream_);
  PTTS_HIP(hipStreamSynchronize(stream_));
  PTTS_HIP(hipFree(tmp));
  return (const uint32_t*)q;
}

void Engine::derive_gemv() {
  // sequential stepping (the B = 1 first-chunk path, no concurrent back part) and frame-pair
  // pipelined stepping (the front part bounds the step): every matrix. Single-frame pipelined
  // stepping (the back part bounds it): qkv and linear1 stay on the LDS-DMA tile, whose smaller
  // register footprint crowds the concurrent back part less (same-box product bench, DESIGN.md §1:
  // pairs 4,093 -> 4,395x with every matrix register-resident, single frames 4,228 -> 4,170x)
  int mask = pipeline_ && nfr_ == 1 ? 2 | 8 | 16 : 31;
  if (probe_env("PTTS_GEMV_MASK")) mask = atoi(probe_env("PTTS_GEMV_MASK"));  // probe builds: A/B runs
  gemv_mask_ = mask;
  struct M {
    const float* w;
    int N, K, bit;
    GemvShape g;
  };
  std::vector<M> mats;
  const GemvShape wide{4, 128};  // qkv / linear1 tile
  const GemvShape outg{1, 32};   // out tile
  for (int l = 0; l < NL; ++l) {
    const Layout::TL& t = L_.fl[l];
    mats.push_back({W(t.in_proj), 3 * D, D, 1, wide});
    mats.push_back({W(t.out_proj), D, D, 2, outg});
    mats.push_back({W(t.l1), FF, D, 4, wide});
    mats.push_back({W(t.l2), D, FF, 8, GemvShape{1, 64}});
  }
  const GemvShape ada{4, 128};  // flow-head adaLN matrix: 0.6365 -> 0.6315 ms
  mats.push_back({W(L_.ada_w), NADA, FD, 16, ada});
  // Code-carrying matrices (weight_quant: int8, fp8_gemm: e4m3) are read from their codes only
  // (k_gemv / k_ffn_fused with WQ != 0 never touch an f32 packed copy), so they get no f32 copy.
  auto scale_of = [&](const float* w) { return fp8_ ? f8map_.at(w).second : q8map_.at(w).second; };
  // linear1 on the whole-K GEMM (gemv_fk: GELU in its epilogue, no split-K slabs, no reduce launch)
  // wherever the register-resident linear1 is used; PTTS_NO_FK (probe builds) keeps the split-K form
  if ((mask & 4) && !probe_env("PTTS_NO_FK") && gemv_fk_supported(1, FF, D)) {
    // linear1 + linear2 as ONE launch (ffn_fused) wherever the whole-K linear1 is used;
    // PTTS_NO_FFN (probe builds) keeps the two launches
    const bool ffn = !probe_env("PTTS_NO_FFN") && ffn_fused_supported(1, D, FF);
    if (ffn) ffn_groups_ = probe_env("PTTS_FFN16") ? 16 : 8;  // probe builds: the 16-group form, for A/B runs
    const int G = ffn_groups_;
    // weight_quant / fp8 engines: both matrices as codes (the fused launch then streams a quarter
    // of the bytes)
    std::vector<std::pair<const uint32_t*, const uint32_t*>> codes(NL, {nullptr, nullptr});
    bool all_codes = ffn;
    for (int l = 0; l < NL && ffn; ++l) {
      const float *w1 = W(L_.fl[l].l1), *w2 = W(L_.fl[l].l2);
      codes[l].first = pack_codes(w1, FF, D, 8, [&](const float* c, float* o) { pack_gemv_fk(c, FF, D, o, stream_); });
      codes[l].second = pack_codes(w2, D, FF, 8, [&](const float* c, float* o) { pack_ffn2(c, G, o, stream_); });
      if (codes[l].first && codes[l].second) ffn8map_[w2] = {{codes[l].first, scale_of(w1)}, {codes[l].second, scale_of(w2)}};
      else all_codes = false;
    }
    const bool f32_copies = !all_codes;
    void* q = nullptr;
    PTTS_HIP(hipMalloc(&q, sizeof(float) * ((f32_copies ? (size_t)NL * FF * D : 0) + FK_A_FLOATS)));  // all written before read
    allocs_.push_back(q);
    float* dst = (float*)q;
    for (int l = 0; l < NL; ++l) {
      if (f32_copies) pack_gemv_fk(W(L_.fl[l].l1), FF, D, dst, stream_);
      fkmap_[W(L_.fl[l].l1)] = f32_copies ? dst : nullptr;  // nullptr: the fused launch reads the codes
      if (f32_copies) dst += (size_t)FF * D;
    }
    hfrag_ = dst;
    if (ffn) {
      void* f = nullptr;
      PTTS_HIP(hipMalloc(&f, sizeof(float) * ((f32_copies ? (size_t)NL * D * FF : 0) + 2 * FFN_HAND_FLOATS)));
      allocs_.push_back(f);
      float* fd = (float*)f;
      for (int l = 0; l < NL; ++l) {
        if (f32_copies) pack_ffn2(W(L_.fl[l].l2), G, fd, stream_);
        ffnmap_[W(L_.fl[l].l2)] = f32_copies ? fd : nullptr;
        if (f32_copies) fd += (size_t)D * FF;
      }
      ffn_hand_ = fd;  // both sets empty (0xFFFFFFFF) before the first launch
      PTTS_HIP(hipMemsetD32Async(ffn_hand_, 0xFFFFFFFFu, 2 * FFN_HAND_FLOATS, stream_));
    }
  }
  std::vector<Gemv> sel;  // (matrix, codes) of every register-resident matrix
  std::vector<const M*> selm;
  size_t total = 0;
  for (const M& m : mats) {
    if (!(mask & m.bit) || !gemv_supported(m.g, m.N, m.K)) continue;
    Gemv gv{nullptr, m.g, m.bit, nullptr, nullptr};
    // weight_quant engines: the int8 codes of a quantized matrix in the same fragment order;
    // fp8_gemm engines: the e4m3 codes of the {4, 128} matrices (qkv, adaLN; W8A8 tiles). An e4m3
    // matrix on another tile (linear2's {1, 64}) gets no register-resident form at all: it stays on
    // k_gemm_fp8 (W8A8), so every fp8 matrix runs fp8 in every stepping mode
    const GemvShape g = m.g;
    const int N = m.N, K = m.K;
    if (!fp8_ || (g.wn == 4 && g.kw == 128)) {
      gv.q8 = pack_codes(m.w, N, K, g.kw / 8, [&](const float* c, float* o) { pack_gemv(c, N, K, g, o, stream_); });
      if (gv.q8) gv.scale = scale_of(m.w);
    } else if (f8map_.count(m.w)) {
      continue;
    }
    if (!gv.q8) total += (size_t)N * K;
    sel.push_back(gv);
    selm.push_back(&m);
  }
  float* dst = nullptr;
  if (total) {
    void* p = nullptr;
    PTTS_HIP(hipMalloc(&p, sizeof(float) * total));  // every element is written by the packing
    allocs_.push_back(p);
    dst = (float*)p;
  }
  for (size_t i = 0; i < sel.size(); ++i) {
    const M& m = *selm[i];
    Gemv gv = sel[i];
    if (!gv.q8) {
      pack_gemv(m.w, m.N, m.K, m.g, dst, stream_);
      gv.packed = dst;
      dst += (size_t)m.N * m.K;
    }
    gvmap_[m.w] = gv;
  }
  PTTS_HIP(hipGetLastError());
  PTTS_HIP(hipStreamSynchronize(stream_));
}

// bf16x6 back part (back_mfma = PTTS_BACK_F32X6): every back-part GEMM / conv weight matrix split
// into its exact three bf16 pieces (split3: hi | mid in W's f32 layout, lo as bf16), padded with
// zero rows to a multiple of 32 (the tiles read rows < Nw). Shapes as build_back multiplies them.
void Engine::derive_split() {
  auto add = [&](size_t off, int N, int K) {
    const int Nw = (N + 31) / 32 * 32;
    void *hm = nullptr, *lo = nullptr;
    PTTS_HIP(hipMalloc(&hm, sizeof(unsigned) * (size_t)Nw * K));
    allocs_.push_back(hm);
    PTTS_HIP(hipMalloc(&lo, sizeof(unsigned short) * (size_t)Nw * K));
    allocs_.push_back(lo);
    if (Nw > N) {
      PTTS_HIP(hipMemsetAsync((unsigned*)hm + (size_t)N * K, 0, sizeof(unsigned) * (size_t)(Nw - N) * K, stream_));
      PTTS_HIP(hipMemsetAsync((unsigned short*)lo + (size_t)N * K, 0, sizeof(unsigned short) * (size_t)(Nw - N) * K,
                              stream_));
    }
    split3(W(off), (long)N * K, (unsigned*)hm, (unsigned short*)lo, stream_);
    split_[W(off)] = {(const unsigned*)hm, (const unsigned short*)lo};
  };
  for (int l = 0; l < MNL; ++l) {
    const Layout::TL& t = L_.mdec[l];
    add(t.in_proj, 3 * MD, MD);
    add(t.out_proj, MD, MD);
    add(t.l1, MFF, MD);
    add(t.l2, MD, MFF);
  }
  add(L_.dc0_w, 512, 7 * 512);
  for (int i = 0, ch = 512; i < 3; ++i, ch /= 2) {
    add(L_.dtr_w[i], RATIOS[i] * (ch / 2), 2 * ch);
    add(L_.dra_w[i], ch / 4, 3 * (ch / 2));
    add(L_.drb_w[i], ch / 2, ch / 4);
  }
  PTTS_HIP(hipGetLastError());
  PTTS_HIP(hipStreamSynchronize(stream_));
}

// A bf16x6 tile reads the split copy of its weight matrix (derive_split)
void Engine::attach_split(GemmArgs& a) const {
  if (!tile_of(a.layout).split_weights()) return;
  auto it = split_.find(a.W);
  PTTS_REQUIRE(it != split_.end(), "bf16x6 tile without a split weight copy");
  a.Whm = it->second.first;
  a.Wlo = it->second.second;
}

void Engine::finalize() {
  PTTS_HIP(hipSetDevice(dev_));
  if (wq_ != QUANT_NONE && q8map_.empty()) derive_int8();
  if (fp8_ && f8map_.empty()) derive_fp8();
  if (gvmap_.empty()) derive_gemv();
  if (back_mfma_ == PTTS_BACK_F32X6 && split_.empty()) derive_split();
  if (!inw_t_) {  // every element is written by the transpose below: no (null-stream) memset
    void* p = nullptr;
    PTTS_HIP(hipMalloc(&p, sizeof(float) * LDIM * D));
    allocs_.push_back(p);
    inw_t_ = (float*)p;
  }
  transpose(W(L_.input_linear), D, LDIM, inw_t_, stream_);
  if (!fh_inw_t_) {  // flow-head input projection transposed ([32][512], the x0 side job)
    void* p = nullptr;
    PTTS_HIP(hipMalloc(&p, sizeof(float) * LDIM * FD));
    allocs_.push_back(p);
    fh_inw_t_ = (float*)p;
  }
  transpose(W(L_.inproj_w), FD, LDIM, fh_inw_t_, stream_);
  if (!fhw_ && head_uniform_stride()) {  // every element is written by the packing below
    void* p = nullptr;
    PTTS_HIP(hipMalloc(&p, sizeof(float) * flow_head_packed_floats()));
    allocs_.push_back(p);
    fhw_ = (float*)p;
  }
  if (fhw_) pack_flow_head(W(L_.rb_w0[0]), W(L_.rb_w2[0]), (long)(L_.rb_w0[1] - L_.rb_w0[0]), W(L_.fin_w), fhw_, stream_);
  // flow-head prelude (f32 engines; the quantized engines' heads stream codes through their own
  // launches): cond | EOS on the whole-K GEMM, the adaLN matrix in the prelude's fragment order
  static_assert(HP_NCOND == NCOND_PAD && HP_NADA == NADA, "head_prelude's shapes are the flow head's");
  if (wq_ == QUANT_NONE && !fp8_ && hfrag_ && gemv_fk_supported(1, NCOND_PAD, D)) {
    if (!hp_w_) {  // every element is written by the packing below
      void* p = nullptr;
      PTTS_HIP(hipMalloc(&p, sizeof(float) * ((size_t)NCOND_PAD * D + (size_t)NADA * FD)));
      allocs_.push_back(p);
      hp_w_ = (float*)p;
    }
    pack_gemv_fk(W(L_.cond_eos_w), NCOND_PAD, D, hp_w_, stream_);
    pack_head_ada(W(L_.ada_w), hp_w_ + (size_t)NCOND_PAD * D, stream_);
  }
  TimeEmbedWeights tw;
  for (int i = 0; i < 2; ++i) {
    tw.l1w[i] = W(L_.te_l1w[i]);
    tw.l1b[i] = W(L_.te_l1b[i]);
    tw.l2w[i] = W(L_.te_l2w[i]);
    tw.l2b[i] = W(L_.te_l2b[i]);
    tw.alpha[i] = W(L_.te_alpha[i]);
  }
  // the time embeddings of every per-row step count n = 1 .. cap (s = i / n, t = (i + 1) / n,
  // mlp.rs:296-319), triangular: the n rows of count n start at row n (n - 1) / 2
  for (int n = 1; n <= lsd_; ++n) time_embeddings(tw, n, temb_tmp_, temb_ + (size_t)temb_row0(n) * FD, stream_);
  rope_table(rope_, max_ctx_, stream_);
  for (int i = 0, ch = MD / 2; i < 3; ++i, ch /= 2)  // bias of the phase-merged transposed convs
    for (int p = 0; p < RATIOS[i]; ++p)
      PTTS_HIP(hipMemcpyAsync(trb_[i] + (size_t)p * ch, W(L_.dtr_b[i]), sizeof(float) * ch, hipMemcpyDeviceToDevice,
                              stream_));
  PTTS_HIP(hipGetLastError());
  PTTS_HIP(hipStreamSynchronize(stream_));
  ready_ = true;
}

void Engine::run_ops(const std::vector<Op>& ops) {
  xh_dirty_ = true;  // the admission's text prefill uses fbm_.x / fbm_.h as scratch
  run_ops_on(ops, stream_);
}

void Engine::run_ops_on(const std::vector<Op>& ops, hipStream_t s) {
  for (const Op& op : ops) {
    op.fn(s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) throw Error(PTTS_ERR_HIP, "launch of " + op.name + " failed: " + hipGetErrorString(e));
  }
}

// int8 code matrices of the quantized FlowLM GEMM weights, derived on the device from the
// blob (so a blob received over RCCL needs nothing else): every Layout::Q8 matrix whose rows
// all carry a scale gets codes; quant_codes checks float(q) * s == W bit for bit.
void Engine::derive_int8() {
  float mode = 0.f;
  PTTS_HIP(hipMemcpy(&mode, blob_ + L_.qmode, sizeof(float), hipMemcpyDeviceToHost));
  PTTS_REQUIRE((int)mode == wq_, "weight blob was packed with a different weight_quant mode");
  std::vector<const Layout::Q8*> use;
  size_t bytes = 0;
  for (const Layout::Q8& q : L_.q8) {
    std::vector<float> s((size_t)q.N);
    PTTS_HIP(hipMemcpy(s.data(), blob_ + q.s, s.size() * sizeof(float), hipMemcpyDeviceToHost));
    if (std::all_of(s.begin(), s.end(), [](float v) { return v > 0.f; })) {
      use.push_back(&q);
      bytes += ((size_t)q.N * q.K + 255) / 256 * 256;
    }
  }
  if (use.empty()) return;
  void* codes = nullptr;
  PTTS_HIP(hipMalloc(&codes, bytes));
  allocs_.push_back(codes);
  int* bad = (int*)dalloc(1);
  size_t off = 0;
  for (const Layout::Q8* q : use) {
    int8_t* c = (int8_t*)codes + off;
    quant_codes(W(q->w), W(q->s), q->N, q->K, c, bad, stream_);
    q8map_[W(q->w)] = {c, W(q->s)};
    off += ((size_t)q->N * q->K + 255) / 256 * 256;
  }
  PTTS_HIP(hipGetLastError());
  int nbad = 0;
  PTTS_HIP(hipMemcpyAsync(&nbad, bad, sizeof(int), hipMemcpyDeviceToHost, stream_));
  PTTS_HIP(hipStreamSynchronize(stream_));
  if (nbad) {
    q8map_.clear();
    throw Error(PTTS_ERR_INVALID, "quantized weights are not on their int8 grid (" + std::to_string(nbad) +
                                      " elements): blob not packed by the quantizer");
  }
}

// e4m3 codes + row scales of the large FlowLM step GEMM weights (the int8 path's set: qkv,
// linear1, linear2, adaLN; >= 2M weights), derived on the device from the f32 blob.
void Engine::derive_fp8() {
  std::vector<const Layout::Q8*> use;
  size_t bytes = 0, nsc = 0;
  for (const Layout::Q8& q : L_.q8)
    if ((long)q.N * q.K >= (2L << 20)) {
      use.push_back(&q);
      bytes += ((size_t)q.N * q.K + 255) / 256 * 256;
      nsc += (size_t)q.N;
    }
  void* codes = nullptr;
  PTTS_HIP(hipMalloc(&codes, std::max<size_t>(bytes, 1)));
  allocs_.push_back(codes);
  float* scales = dalloc(nsc);
  size_t off = 0, so = 0;
  for (const Layout::Q8* q : use) {
    uint8_t* c = (uint8_t*)codes + off;
    fp8_codes(W(q->w), q->N, q->K, c, scales + so, stream_);
    f8map_[W(q->w)] = {c, scales + so};
    off += ((size_t)q->N * q->K + 255) / 256 * 256;
    so += (size_t)q->N;
  }
  PTTS_HIP(hipGetLastError());
  PTTS_HIP(hipStreamSynchronize(stream_));
}

// ------------------------------------------------------------------ op builders
void Engine::linear_split(std::vector<Op>& ops, const std::string& name, const float* X, long ldx, int M,
                          const float* Wt, int N, int K, int* S_out, const FlowBufs& fb) {
  PTTS_REQUIRE(K % 32 == 0, "GEMM K must be a multiple of 32");
  int S = pick_splits(M, N, K);
  int layout = TILE_KSPLIT_4W, tail = 0;
  // wide skinny GEMMs (FlowLM qkv/ff1, flow-head adaLN): 32x128 LDS-DMA tiles, 8-way split-K
  // (tools/gemm_bench.hip on MI355X: qkv 6.7 -> 6.3 us, ff1 7.9 -> 6.5 us, ada 10.1 -> 8.7 us)
  if (M <= 64 && N >= 3072) {
    layout = TILE_GLDS_32x128;  // 2-buffer LDS (40 KB) co-resides with the back part
    S = std::max(1, std::min(8, K / 64));
  } else if (M >= 256) {  // prefill passes (text admission, M = 48 rows per slot): MFMA-bound,
    // LDS-DMA tiles with the DMAs interleaved between the MFMAs and a split tail (the tiles past
    // whole rounds of the CUs' workgroup slots run as K slices; tools/mm_bench.hip at M = 1536,
    // against rocBLAS fp32 on the same box: qkv 108 / 111, out 88 / 98, ff1 112 / 125, ff2 117 /
    // 122 TF/s): 128x64, two per CU, 4 slices; linear1 128x64 one per CU, 2 slices
    layout = N >= 4096 && K <= 1024 ? TILE_ILV_128x64 : TILE_ILV_128x64_2CU;
    tail = N >= 4096 && K <= 1024 ? 2 : 4;
    S = 1;
  } else if (M <= 64 && K >= 4096) {  // FlowLM ff2: 8 slabs (tools/gemm_bench.hip flow.ff2: 8.5 -> 7.3 us)
    S = 8;
  } else if (M <= 64 && N <= 512 && K == 512) {  // flow-head MLPs: 8 waves, 8 slabs (head.mlp: 3.9 -> 3.4 us)
    layout = TILE_KSPLIT_8W;
    S = 8;
  }
  // quantized FlowLM weights on the step path: stream int8 codes (k_gemm_w8, 32x64 tiles, the
  // smallest power-of-two split reaching 256 workgroups with >= 4 K chunks per slice). Only the
  // large matrices (qkv, ff1, ff2, adaLN; >= 2M weights): below that the launch is latency-bound
  // and the f32 copy of the same values is as fast (tools/w8_probe.py). Prefill passes
  // (M >= 256) keep the f32 copy too: they are MFMA-bound.
  auto gv = gvmap_.find(Wt);
  if (gv != gvmap_.end() && M <= 64 && (gemv_mask_ & gv->second.bit)) {  // register-resident weights (derive_gemv)
    const GemvShape g = gv->second.g;
    const float* P = gv->second.packed;
    const uint32_t* q8 = gv->second.q8;
    const float* sc = gv->second.scale;
    const int Sg = K / g.ks();
    PTTS_REQUIRE((size_t)Sg * M * N <= fb.pcap, "split-K partial buffer too small");
    float* part = fb.partial;
    const bool f8 = fp8_ && q8;
    ops.push_back({name, [=](hipStream_t s) { gemv_splitk(X, ldx, M, N, K, P, g, part, s, q8, sc, f8); }, 2.0 * M * N * K,
                   (q8 ? 1.0 * N * K + 4.0 * N : 4.0 * N * K) + 4.0 * ((double)M * K + (double)Sg * M * N)});
    *S_out = Sg;
    return;
  }
  auto f8 = f8map_.find(Wt);
  const bool wf8 = f8 != f8map_.end() && M <= 64;
  if (wf8) {  // fp8 W8A8 (k_gemm_fp8): 32x64 tiles, >= 256 workgroups, K slice <= FP8_KSLICE_MAX
    layout = TILE_KSPLIT_4W;
    const int tiles = ((N + 63) / 64) * ((M + 31) / 32), nch = K / 32;
    S = 1;
    while (S < 16 && tiles * S < 256 && nch / (2 * S) >= 4) S *= 2;
    while ((nch + S - 1) / S > FP8_KSLICE_MAX / 32) ++S;
  }
  auto q8 = q8map_.find(Wt);
  const bool w8 = q8 != q8map_.end() && M <= 64 && (long)N * K >= (2L << 20);
  if (w8) {
    layout = TILE_KSPLIT_4W;
    const int tiles = ((N + 63) / 64) * ((M + 31) / 32);
    S = 1;
    while (S < 16 && tiles * S < 256 && (K / 32) / (2 * S) >= 4) S *= 2;
  }
  if (!w8 && !wf8) tile_override(name, layout, S);
  while (S > 1 && (size_t)S * M * N > fb.pcap) --S;
  PTTS_REQUIRE((size_t)S * M * N <= fb.pcap, "split-K partial buffer too small");
  GemmArgs a = dense_gemm(layout, M, N, K, X, ldx, Wt);
  if (w8) {
    a.Wq = q8->second.first;
    a.wscale = q8->second.second;
  }
  if (wf8) {
    PTTS_REQUIRE((K / 32 + S - 1) / S <= FP8_KSLICE_MAX / 32, "fp8 GEMM K slice too long");
    a.Wf8 = f8->second.first;
    a.wscale = f8->second.second;
  }
  a.S = S;
  a.partial = fb.partial;
  if (tail > 0 && S == 1 && !w8 && !wf8) {
    a.tail_S = tail;
    a.tail_slab = fb.tslab;
    a.tail_cap = fb.tail_cap;
    a.tickets = fb.tickets;
    a.tickets_cap = TICKETS;
  }
  // FlowLM / flow-head step weights are read once per step: non-temporal loads on the LDS-DMA
  // tiles (step -1.1 %; the 4-wave 32x32 register tile keeps default-policy loads)
  a.w_nt = M <= 64 && layout != TILE_KSPLIT_4W;
  a.front = 1;  // FlowLM / flow-head GEMMs (and the prefill passes, on the same stream)
  ops.push_back({name, [a, S](hipStream_t s) { gemm(a, S, s); }, 2.0 * M * N * K,
                 (w8 || wf8 ? (double)N * K + 4.0 * N : 4.0 * N * K) + 4.0 * ((double)M * K + (double)S * M * N)});
  *S_out = S;
}

// Algorithmic cost of a row-reduce launch (HBM-bound): the S slabs, the operands it reads per row
// (bias, gate, residual, LayerNorm affine, modulation) and every row it stores, plus the side jobs.
static Op rr_op(const std::string& name, const RowReduceArgs& a) {
  const double mn = (double)a.M * a.N;
  double f = mn * (a.S + 1 + (a.act ? 8 : 0) + (a.ln ? 8 : 0));
  double b = mn * a.S + (a.bias ? a.N : 0) + (a.gate ? (a.ldg ? mn : a.N) : 0) + (a.R ? mn : 0) + (a.Y ? mn : 0) +
             (a.Y2 ? mn : 0) + (a.euler ? 2.0 * a.M * 32 : 0);
  if (a.ln) b += mn + (a.ln_w ? 2.0 * a.N : 0) + (a.mshift ? 2.0 * mn : 0);
  if (a.fhm) b += mn * 2.0 / 3.0;  // the fragment-order copy of the shift / scale columns
  if (a.fill) b += 4.0 * a.fill_n4;
  if (a.x0_hx) {  // x0 = cur W_in^T + b_in for x0_B rows
    b += (double)a.x0_B * (32 + 512) + 32.0 * 512;
    f += 2.0 * a.x0_B * 32 * 512;
  }
  return Op{name, [a](hipStream_t s) { row_reduce(a, s); }, f, 4.0 * b};
}

// The row-reduce epilogue of the split GEMM just emitted, as its own launch (an in-launch split-K
// combine by the last-arriving workgroup measured slower on every front GEMM: ff2 43 vs 13 us with
// the LayerNorm row finisher, ff1 15.6 vs 11.4 us tile-local).
void Engine::push_rr(std::vector<Op>& ops, const std::string& name, const RowReduceArgs& r) {
  RowReduceArgs a = r;
  a.front = 1;  // the FlowLM / flow-head reduces (the back part's go through rr_op directly)
  ops.push_back(rr_op(name, a));
}

void Engine::dense_op(std::vector<Op>& ops, const std::string& name, const float* X, int M, const float* Wt, int N,
                      int K, const float* bias, int act, const float* rscale, const float* R, float* Y, int layout) {
  int ks = 1;
  tile_override(name, layout, ks);
  PTTS_REQUIRE(K % tile_of(layout).bk == 0, "GEMM K must be a multiple of the tile's BK");
  GemmArgs a = dense_gemm(layout, M, N, K, X, K, Wt);
  a.S = 1;
  a.bias = bias;
  a.act = act;
  a.rscale = rscale;
  a.R = R;
  a.ldr = N;
  a.Y = Y;
  a.ldy = N;
  attach_split(a);
  ops.push_back({name, [a](hipStream_t s) { gemm(a, 1, s); }, 2.0 * M * N * K,
                 4.0 * ((double)N * K + (double)M * K + (double)M * N * (R ? 2 : 1))});
}

void Engine::conv_op(std::vector<Op>& ops, const std::string& name, const float* X, int B, int T_in, int cin,
                     const float* H, int P, int stride, int elu, const float* Wt, int cout, int ktaps, int phases,
                     const float* bias, const float* R, float* Y, int T_out, int tstride, int layout, int elu_out,
                     float* Y2, int ksplit, float* slabs, size_t slab_cap) {
  tile_override(name, layout, ksplit);
  const TileInfo& tile = tile_of(layout);
  PTTS_REQUIRE(cin % tile.bk == 0, "conv cin must be a multiple of the tile's BK");
  // ksplit > 1: single-phase conv on an LDS-DMA tile, K split into ksplit partial slabs in the
  // caller's slab buffer; the caller adds the row-reduce epilogue
  PTTS_REQUIRE(ksplit == 1 || (phases == 1 && tile.lds_dma()), "K-split convs need a single-phase LDS-DMA tile");
  GemmArgs a{};
  a.mode = 1;
  a.layout = layout;
  a.Tq = T_in / stride;
  a.M = B * a.Tq;
  a.N = cout;
  a.K = ktaps * cin;
  a.Nw = (cout + 31) / 32 * 32;
  a.X = X;
  a.ldx = cin;
  a.H = H;
  a.P = P;
  a.T_in = T_in;
  a.stride_in = stride;
  a.cin = cin;
  a.elu_in = elu;
  a.W = Wt;
  a.w_phase_stride = (long)cout * ktaps * cin;
  a.S = 1;
  a.bias = bias;
  a.R = R;
  a.ldr = cout;
  a.Y = Y;
  a.ldy = cout;
  a.T_out = T_out;
  a.out_tstride = tstride;
  a.elu_out = elu_out;
  a.Y2 = Y2;
  const int nph = phases;
  attach_split(a);
  if (ksplit > 1) {
    PTTS_REQUIRE((size_t)ksplit * a.M * a.N <= slab_cap, "back split-K slab buffer too small");
    a.S = ksplit;
    a.partial = slabs;
    phases = ksplit;  // grid z
  }
  ops.push_back({name, [a, phases](hipStream_t s) { gemm(a, phases, s); }, 2.0 * a.M * a.N * a.K * nph,
                 4.0 * ((double)nph * a.N * a.K + (double)B * T_in * cin +
                        (double)B * T_out * cout * ((R ? 2 : 1) + (Y2 ? 1 : 0)))});
}

// FlowLM transformer layers over M rows of the workspace fb (fb.x holds the residual stream, fb.h =
// norm1_0(fb.x)). StreamingTransformerLayer::forward (transformer.rs:66-90).
void Engine::flow_layers(std::vector<Op>& ops, int M, RowMap map, bool step, bool out_norm, const std::string& tag,
                         const FlowBufs& fb, float* align_out) {
  // (the step's fused launches hand over through hfrag_ / ffn_hand_, of which there is one set)
  PTTS_REQUIRE(!step || &fb == &fbm_, "step passes run on the engine's own buffers");
  for (int l = 0; l < NL; ++l) {
    const Layout::TL& t = L_.fl[l];
    const std::string p = tag + ".l" + std::to_string(l);
    KvStore kv = fb.kv;
    kv.base += (long)l * fb.kv_layer;
    if (kv.pre) kv.layer = l;  // shared voice prefixes (fbm_)
    int S = 1;
    linear_split(ops, p + ".qkv_gemm", fb.h, D, M, W(t.in_proj), 3 * D, D, &S, fb);
    if (step) {  // step: slab sum + RoPE + KV append fused into the attention kernel
      const float* P = fb.partial;
      float* O = fb.o;
      const float* rope = rope_;
      // K and V of every head over the cached positions the launch reads (8,192 B per position):
      // each row's own positions, plus ONE copy of every distinct shared voice prefix (the rows of
      // a voice read its cache, KvStore::pre: plan_kvu_), the QKV slabs, the appended K/V and the
      // output row; QK^T + PV = 4,096 flops per position and row
      const double L = plan_ctx_ > 0 ? plan_ctx_ : max_ctx_ / 2.0;
      const double kvu = plan_kvu_ > 0 ? plan_kvu_ : M * L;
      ops.push_back({p + ".attention", [=](hipStream_t s) { attention_step_qkv(P, S, M, NH, map, kv, rope, O, s); },
                     (double)M * 4096.0 * L,
                     8192.0 * kvu + (double)M * (4.0 * (S * 3.0 * D + 2.0 * D + D) + 64.0 * 4 * 2)});
      if (align_out && l == align_layer_) {
        // the text-attention rows of this layer (section 26), while the query's slabs are still in
        // fb.partial (out_gemm overwrites them) and this position's keys in the store. Stream order:
        // not a parallel branch. Cost for rows of n text tokens over h selected heads: the keys
        // (256 B each), the q slabs and the RoPE row in, ALIGN_ROW words out; a 64-term dot per key
        // and ~8 flops per softmax element. Stated for the rows in the stage at the time of the call
        // (none: the launch writes one count per row).
        AlignArgs a{};
        a.P = P;
        a.S = S;
        a.M = M;
        a.nh = NH;
        a.pos = map.pos_arr;
        a.kv = kv;
        a.rope = rope;
        a.tab = align_tab_;
        a.head_mask = align_mask_;
        a.out = align_out;
        double rows = 0, keys = 0;
        for (int b = 0; b < M; ++b)
          if (slot_align_[b]) rows += 1, keys += slot_align_[b];
        const double h = __builtin_popcount(align_mask_);
        ops.push_back({p + ".align", [=](hipStream_t s) { align_step(a, s); }, h * keys * (128.0 + 8.0),
                       h * (256.0 * keys + rows * 4.0 * (S * 64.0 + 64.0)) + rows * 4.0 * ALIGN_ROW +
                           (M - rows) * 4.0 + M * 12.0});
      }
    } else {
      {
        const float* P = fb.partial;
        float* Q = fb.q;
        ops.push_back({p + ".qkv_rope", [=](hipStream_t s) { qkv_rope_append(P, S, nullptr, M, NH, map, kv, Q, s); }});
      }
      const float* Q = fb.q;
      float* O = fb.o;
      RowMap am = map;  // compact admission: the attention runs on the padded 16-row groups
      int Ma = M;
      if (map.ptab) {
        am.tab = map.ptab;
        Ma = map.mpad;
      }
      ops.push_back({p + ".attention", [=](hipStream_t s) { attention(Q, Ma, NH, am, kv, 0, O, s); }});
    }
    auto rr = [&](const std::string& name, int S2, int N, int act, bool resid, float* Y, const float* lnw,
                  const float* lnb, bool ln, float* Hout, float* Hfrag = nullptr, float* fill = nullptr,
                  long fill_n4 = 0) {
      RowReduceArgs a{};
      a.Hfrag = Hfrag;
      a.fill = fill;
      a.fill_n4 = fill_n4;
      a.P = fb.partial;
      a.S = S2;
      a.M = M;
      a.N = N;
      a.act = act;
      if (resid) {
        a.R = fb.x;
        a.ldr = D;
      }
      a.Y = Y;
      a.ldy = N;
      a.ln = ln ? 1 : 0;
      a.ln_w = lnw;
      a.ln_b = lnb;
      a.eps = 1e-5f;
      a.Hout = Hout;
      a.ldh = N;
      push_rr(ops, name, a);
    };
    linear_split(ops, p + ".out_gemm", fb.o, D, M, W(t.out_proj), D, D, &S, fb);
    // step passes with the whole-K linear1 (gemv_fk): the out reduce also stores norm2's output in
    // its A-fragment order, and linear1 applies GELU in its own epilogue (no slabs, no reduce)
    auto fk = step && gemv_fk_supported(M, FF, D) ? fkmap_.find(W(t.l1)) : fkmap_.end();
    const bool use_fk = fk != fkmap_.end() && hfrag_;
    rr(p + ".out_reduce_ln2", S, D, ACT_NONE, true, fb.x, W(t.n2w), W(t.n2b), true, fb.h, use_fk ? hfrag_ : nullptr);
    auto ffn = use_fk && ffn_hand_ ? ffnmap_.find(W(t.l2)) : ffnmap_.end();
    if (ffn != ffnmap_.end()) {
      // linear1 + GELU + linear2 in one launch (16 K slices of linear2 into the slabs): layer l uses
      // hand-off set l % 2 and empties the other for layer l + 1 (the last layer's launch empties
      // set 0 for the next step's first, NL even)
      static_assert(NL % 2 == 0, "the fused FFN's hand-off sets alternate by layer");
      const float *A = hfrag_, *P1 = fk->second, *P2 = ffn->second;
      float *hand = ffn_hand_, *Pp = fb.partial;
      int* err = herr_;
      const int set = l & 1;
      const int groups = ffn_groups_;
      auto f8 = ffn8map_.find(W(t.l2));  // weight_quant engines: int8 codes of both matrices
      const uint32_t *Q1 = nullptr, *Q2 = nullptr;
      const float *s1 = nullptr, *s2 = nullptr;
      if (f8 != ffn8map_.end()) {
        Q1 = f8->second.first.first;
        s1 = f8->second.first.second;
        Q2 = f8->second.second.first;
        s2 = f8->second.second.second;
      }
      const bool e4m3 = fp8_ && Q1;
      Op op{p + ".ffn", [=](hipStream_t s) { ffn_fused(A, M, P1, P2, groups, hand, set, Pp, err, s, Q1, s1, Q2, s2, e4m3); },
            2.0 * M * FF * D * 2,
            (Q1 ? 2.0 * FF * D + 8.0 * (FF + D) : 8.0 * FF * D) + 4.0 * ((double)M * D + (double)groups * M * D)};
      // an isolated replay (time_op, overlap_probe) finds its set empty again
      op.prep = [hand](hipStream_t s) { PTTS_HIP(hipMemsetD32Async(hand, 0xFFFFFFFFu, 2 * FFN_HAND_FLOATS, s)); };
      ops.push_back(op);
      S = groups;
    } else {
      if (use_fk) {
        const float* Pk = fk->second;
        const float* A = hfrag_;
        float* U = fb.u;
        ops.push_back({p + ".ff1_gemm", [=](hipStream_t s) { gemv_fk(A, M, FF, Pk, nullptr, ACT_GELU, U, FF, s); },
                       2.0 * M * FF * D, 4.0 * ((double)FF * D + (double)M * D + (double)M * FF)});
      } else {
        linear_split(ops, p + ".ff1_gemm", fb.h, D, M, W(t.l1), FF, D, &S, fb);
        rr(p + ".ff1_reduce_gelu", S, FF, ACT_GELU, false, fb.u, nullptr, nullptr, false, nullptr);
      }
      linear_split(ops, p + ".ff2_gemm", fb.u, FF, M, W(t.l2), D, FF, &S, fb);
    }
    if (l + 1 < NL)
      rr(p + ".ff2_reduce_ln1", S, D, ACT_NONE, true, fb.x, W(L_.fl[l + 1].n1w), W(L_.fl[l + 1].n1b), true, fb.h);
    else {
      // ahead of the head prelude: out_norm's rows also in its A-fragment order, and its hand-off
      // regions emptied (those of the cap: the run length is the front's, not this pass's)
      const bool pre = step && out_norm && use_head_prelude(M);
      const long n4 = (long)lsd_ * ((M + 15) / 16) * HP_REGION_FLOATS / 4;
      rr(p + ".ff2_reduce_outnorm", S, D, ACT_NONE, true, fb.x, W(L_.out_norm_w), W(L_.out_norm_b), out_norm, fb.h,
         pre ? hfrag_ : nullptr, pre ? hp_hand_ : nullptr, pre ? n4 : 0);
    }
  }
}

// Prefill T rows already in fb.x into slot `slot` at positions p0.. (tts_model.rs:580-599, 958-964).
void Engine::prefill_rows(std::vector<Op>& ops, int slot, int T, int p0, const FlowBufs& fb) {
  {
    float *x = fb.x, *h = fb.h;
    const float* w = W(L_.fl[0].n1w);
    const float* b = W(L_.fl[0].n1b);
    ops.push_back({"prefill.ln1", [=](hipStream_t s) { layernorm(x, D, h, D, T, D, w, b, 1e-5f, s); }});
  }
  RowMap map{slot, T, p0, nullptr};
  flow_layers(ops, T, map, false, false, "prefill", fb);
}

// The persistent flow-head launch needs <= 128 rows and ResBlock tensors at one uniform stride
// in the packed blob (pack_weights lays the six blocks out identically).
bool Engine::use_head_chain(int B) const {
  if (!flow_head_fits(B)) return false;
  // every workgroup spins on counters the others bump: all of them must be resident at once
  if (flow_head_grid(B) > head_resident_) return false;
  return head_uniform_stride();
}

// One launch for the head's prelude (head_prelude): f32 engines (hp_w_), at most 32 rows, ahead
// of the persistent chain (whose x0 and region side jobs it carries).
bool Engine::use_head_prelude(int B) const {
  return hp_w_ && head_prelude_supported(B, 1) && gemv_fk_supported(B, NCOND_PAD, D) && use_head_chain(B);
}

bool Engine::head_uniform_stride() const {
  const long s = (long)(L_.rb_w0[1] - L_.rb_w0[0]);
  for (int i = 1; i < FDEPTH; ++i)
    if ((long)(L_.rb_lnw[i] - L_.rb_lnw[i - 1]) != s || (long)(L_.rb_lnb[i] - L_.rb_lnb[i - 1]) != s ||
        (long)(L_.rb_w0[i] - L_.rb_w0[i - 1]) != s || (long)(L_.rb_b0[i] - L_.rb_b0[i - 1]) != s ||
        (long)(L_.rb_w2[i] - L_.rb_w2[i - 1]) != s || (long)(L_.rb_b2[i] - L_.rb_b2[i - 1]) != s)
      return false;
  return true;
}

// FRONT part of a step (FlowLM + flow head) for rows [0, B), handing its frame to buffer `hb`.
// It runs lsd_run Euler steps (lsd_run_for: >= the count of every row of [0, B) that may be active).
void Engine::build_front(std::vector<Op>& ops, int B, int hb, int lsd_run) {
  PTTS_REQUIRE(lsd_run >= 1 && lsd_run <= lsd_, "lsd_run outside [1, cap]");
  int S = 1;
  // ---- FlowLM step (flow_lm.rs:98-164): input_linear -> transformer -> out_norm. The input
  // projection + norm1 of layer 0 (fbm_.x, fbm_.h) were computed by the previous step's front_commit,
  // or by refresh_xh() after anything else wrote them or lat_in_.
  const FlowBufs& fb = fbm_;
  flow_layers(ops, B, RowMap{0, 1, 0, fpos_}, true, true, "flow", fb, align_ ? align_block(hb) : nullptr);
  // ---- flow head (mlp.rs:215-383): cond_embed | out_eos, EOS bookkeeping, noise, adaLN
  // modulations of all lsd steps: one launch (head_prelude) ahead of the chain, or four
  if (use_head_prelude(B)) {
    const int RG = (B + 15) / 16;
    const size_t r0 = (size_t)(RG * 16) * FD;  // floats per hand-off region of the chain
    HeadPreludeArgs a{};
    a.B = B;
    a.lsd = lsd_run;
    a.lsd_cap = lsd_;
    a.A = hfrag_;
    a.Pc = hp_w_;
    a.cbias = W(L_.cond_eos_b);
    a.temb = temb_;
    a.st = st_;
    a.eos_out = eos_;
    a.cur = cur_;
    a.hand = hp_hand_;
    a.Pa = hp_w_ + (size_t)NCOND_PAD * D;
    a.abias = W(L_.ada_b);
    a.mods = mods_;
    a.fhm = fhm_;
    a.x0_w = fh_inw_t_;
    a.x0_b = W(L_.inproj_b);
    a.x0_hx = hx_;
    a.fill = hx_ + r0;
    a.fill_n4 = (long)((hx_floats(B, lsd_run) - r0) / 4);  // the regions of this run, not of the cap
    a.err = herr_;
    const double mn = (double)lsd_run * B * NADA, hand = (double)lsd_run * RG * HP_REGION_FLOATS;
    // weights, biases and the A fragment in; EOS, cur, mods and the shift / scale copy out; the
    // hand-off written and read; x0 and the emptied regions (as the adaLN reduce counted them)
    Op op{"head.prelude", [a](hipStream_t s) { head_prelude(a, s); },
          2.0 * B * NCOND_PAD * D + 2.0 * lsd_run * B * NADA * FD + 2.0 * B * LDIM * FD + 4.0 * lsd_run * B * FD,
          4.0 * ((double)NCOND_PAD * D + NCOND_PAD + (double)FK_A_FLOATS + (double)NADA * FD + NADA + lsd_run * FD +
                 B * (LDIM + 1.0) + 2.0 * hand + mn + mn * 2.0 / 3.0 + (double)B * (LDIM + FD) + (double)LDIM * FD +
                 4.0 * a.fill_n4)};
    // an isolated replay (time_op, overlap_probe) finds its regions empty again
    float* hh = hp_hand_;
    const size_t nh = (size_t)lsd_run * RG * HP_REGION_FLOATS;
    op.prep = [hh, nh](hipStream_t s) { PTTS_HIP(hipMemsetD32Async(hh, 0xFFFFFFFFu, nh, s)); };
    ops.push_back(op);
  } else {
    linear_split(ops, "head.cond_eos_gemm", fb.h, D, B, W(L_.cond_eos_w), NCOND, D, &S, fb);
    PTTS_REQUIRE(S <= FLOW_COND_MAX_SLABS, "head.flow_cond sums at most 16 split-K slabs");
    {
      const float* P = fb.partial;
      const float* bias = W(L_.cond_eos_b);
      const float* temb = temb_;
      const int lsd = lsd_run, cap = lsd_;
      SlotState* st = st_;
      float *ys = ysilu_, *cur = cur_, *eos = eos_;
      ops.push_back(
          {"head.flow_cond", [=](hipStream_t s) { flow_cond(P, S, B, bias, temb, lsd, cap, st, ys, cur, eos, s); },
           (double)B * NCOND * (S + 1) + 4.0 * lsd * B * FD,
           4.0 * ((double)S * B * NCOND + NCOND + lsd * FD + lsd * (double)B * FD + B * (LDIM + 1.0))});
    }
    // all adaLN modulations of all lsd steps in one GEMM (mlp.rs:322-368)
    linear_split(ops, "head.ada_gemm", ysilu_, FD, lsd_run * B, W(L_.ada_w), NADA, FD, &S, fb);
    {
      RowReduceArgs a{};
      a.P = fb.partial;
      a.S = S;
      a.M = lsd_run * B;
      a.N = NADA;
      a.bias = W(L_.ada_b);
      a.Y = mods_;
      a.ldy = NADA;
      if (use_head_chain(B)) {  // side jobs: x0 into hand-off region 0, empty the other regions
        const size_t r0 = (size_t)((B + 15) / 16 * 16) * FD;  // floats per hand-off region
        a.fill = hx_ + r0;
        a.fill_n4 = (long)((hx_floats(B, lsd_run) - r0) / 4);  // the regions of this run, not of the cap
        a.x0_cur = cur_;
        a.x0_w = fh_inw_t_;
        a.x0_b = W(L_.inproj_b);
        a.x0_hx = hx_;
        a.x0_B = B;
        a.fhm = fhm_;
        a.fhm_B = B;
      }
      push_rr(ops, "head.ada_reduce", a);
    }
  }
  // lsd_decode Euler steps (flow_lm.rs:7-22) over ResBlocks (mlp.rs:146-213): one persistent
  // launch (k_flow_head) for the whole chain, or 28 GEMM + row-reduce launches per step
  if (use_head_chain(B)) {
    FlowHeadArgs f{};
    f.B = B;
    f.lsd = lsd_run;
    f.st = st_;
    f.cur = cur_;
    f.mods = mods_;
    f.ldm = NADA;
    f.in_w = W(L_.inproj_w);
    f.in_b = W(L_.inproj_b);
    f.lnw = W(L_.rb_lnw[0]);
    f.lnb = W(L_.rb_lnb[0]);
    f.w0 = W(L_.rb_w0[0]);
    f.b0 = W(L_.rb_b0[0]);
    f.w2 = W(L_.rb_w2[0]);
    f.b2 = W(L_.rb_b2[0]);
    f.blk = (long)(L_.rb_w0[1] - L_.rb_w0[0]);
    f.fin_w = W(L_.fin_w);
    f.fin_b = W(L_.fin_b);
    f.wp = fhw_;
    f.fhm = fhm_;
    f.hx = hx_;
    f.x0_ready = 1;
    f.ctr = hctr_;
    f.err = herr_;
    f.dbg = probe_env("PTTS_HEAD_DBG") ? (unsigned long long*)strtoull(probe_env("PTTS_HEAD_DBG"), nullptr, 0) : nullptr;
    const double fl = 2.0 * lsd_run * B * ((double)FD * LDIM + 2.0 * FDEPTH * FD * FD + (double)LDIM * FD);
    const double by = 4.0 * ((double)FD * LDIM + 2.0 * FDEPTH * FD * FD + (double)LDIM * FD) +
                      4.0 * lsd_run * B * ((double)FDEPTH * 3 * FD + 2 * FD);
    // isolated replays: re-empty the regions and recompute x0 (the adaLN reduce's side jobs)
    float* hx = hx_;
    const size_t nhx = hx_floats(B, lsd_run);
    const float *cur = cur_, *iw = fh_inw_t_, *ib = W(L_.inproj_b);
    Op op{"head.chain", [f](hipStream_t s) { flow_head(f, s); }, fl, by};
    op.prep = [hx, nhx, cur, iw, ib, B](hipStream_t s) {
      PTTS_HIP(hipMemsetD32Async(hx, 0xFFFFFFFFu, nhx, s));
      flow_head_x0(cur, iw, ib, hx, B, s);
    };
    ops.push_back(op);
  }
  for (int st = 0; st < lsd_run && !use_head_chain(B); ++st) {
    const float* mods = mods_ + (size_t)st * B * NADA;
    const std::string p = "head.s" + std::to_string(st);
    linear_split(ops, p + ".inproj_gemm", cur_, LDIM, B, W(L_.inproj_w), FD, LDIM, &S, fb);
    {
      RowReduceArgs a{};
      a.P = fb.partial;
      a.S = S;
      a.M = B;
      a.N = FD;
      a.bias = W(L_.inproj_b);
      a.Y = xf_;
      a.ldy = FD;
      a.ln = 1;
      a.ln_w = W(L_.rb_lnw[0]);
      a.ln_b = W(L_.rb_lnb[0]);
      a.eps = 1e-6f;
      a.mshift = mods + 0;
      a.mscale = mods + FD;
      a.ldm = NADA;
      a.Hout = hf_;
      a.ldh = FD;
      push_rr(ops, p + ".inproj_reduce", a);
    }
    for (int i = 0; i < FDEPTH; ++i) {
      const std::string pb = p + ".rb" + std::to_string(i);
      {
        linear_split(ops, pb + ".mlp0_gemm", hf_, FD, B, W(L_.rb_w0[i]), FD, FD, &S, fb);
        RowReduceArgs a{};
        a.P = fb.partial;
        a.S = S;
        a.M = B;
        a.N = FD;
        a.bias = W(L_.rb_b0[i]);
        a.act = ACT_SILU;
        a.Y = uf_;
        a.ldy = FD;
        push_rr(ops, pb + ".mlp0_reduce", a);
      }
      linear_split(ops, pb + ".mlp2_gemm", uf_, FD, B, W(L_.rb_w2[i]), FD, FD, &S, fb);
      {
        RowReduceArgs a{};
        a.P = fb.partial;
        a.S = S;
        a.M = B;
        a.N = FD;
        a.bias = W(L_.rb_b2[i]);
        a.gate = mods + (size_t)i * 3 * FD + 2 * FD;
        a.ldg = NADA;
        a.R = xf_;
        a.ldr = FD;
        a.Y = xf_;
        a.ldy = FD;
        a.ln = 1;
        a.eps = 1e-6f;
        if (i + 1 < FDEPTH) {
          a.ln_w = W(L_.rb_lnw[i + 1]);
          a.ln_b = W(L_.rb_lnb[i + 1]);
          a.mshift = mods + (size_t)(i + 1) * 3 * FD;
          a.mscale = mods + (size_t)(i + 1) * 3 * FD + FD;
        } else {  // FinalLayer: non-affine LN + final adaLN (mlp.rs:182-213)
          a.mshift = mods + (size_t)FDEPTH * 3 * FD;
          a.mscale = mods + (size_t)FDEPTH * 3 * FD + FD;
        }
        a.ldm = NADA;
        a.Hout = hf_;
        a.ldh = FD;
        push_rr(ops, pb + ".mlp2_reduce", a);
      }
    }
    linear_split(ops, p + ".final_gemm", hf_, FD, B, W(L_.fin_w), LDIM, FD, &S, fb);
    {
      RowReduceArgs a{};
      a.P = fb.partial;
      a.S = S;
      a.M = B;
      a.N = LDIM;
      a.bias = W(L_.fin_b);
      a.euler = cur_;
      a.euler_st = st_;
      a.euler_step = st;
      push_rr(ops, p + ".euler", a);
    }
  }
  // ---- EOS rule, frame flags, hand-off of the frame to the back part, next backbone input
  {
    FrontCommitArgs c{};
    c.B = B;
    c.st = st_;
    c.eos = eos_;
    c.cur = cur_;
    c.lat_in = lat_in_;
    c.lat_out = lat_out_[hb];
    c.eos_out = eos_out_[hb];
    c.flags = flags_[hb];
    c.fpos = fpos_;
    c.Wt = inw_t_;
    c.lnw = W(L_.fl[0].n1w);
    c.lnb = W(L_.fl[0].n1b);
    c.x = fb.x;
    c.h = fb.h;
    c.err_dev = herr_;
    c.err_host = h_err_;
    c.n_zero = nfr_ > 1 ? max_slots_ - B : 0;
    ops.push_back({"front_commit", [c](hipStream_t s) { front_commit(c, s); }, 2.0 * B * D * LDIM,
                   (double)B * (sizeof(SlotState) * 2 + 4.0 * (1 + 3 * LDIM + 1 + 2 + 2 + 2 * D)) +
                       4.0 * ((double)D * LDIM + 2 * D)});
  }
}

// Tiles of the back part's GEMMs and convs at B >= 16 (the MFMA-bound shapes), one row per launch:
// tile id (kernels.h PTTS_TILES) and split-K slices. Chosen from tools/mm_bench.hip
// (each launch alone on the chip, B = 32) and A/B runs of the pipelined step, where the back part
// shares every CU with the latency-bound front part. Pipelined split-K at most 2
// since round 5 (the front part bounds the step, and 4 slices' slab traffic slowed it: 0.549 ->
// 0.530 ms, profiles/r05/back_splits_ab.txt). Below B = 16 every GEMM runs on the 32x32 register
// tile (TILE_KSPLIT_4W) with the split-K noted at the launch.
struct BackTile {
  int layout, splits;
};
static BackTile back_tile(const std::string& op, bool pipeline) {
  static const struct {
    const char* op;
    BackTile seq, pipe;
  } table[] = {
      {"mimi.qkv", {TILE_ILV_64x64_2CU, 1}, {TILE_ILV_64x64_2CU, 1}},
      {"mimi.out", {TILE_ILV_64x64_2CU, 4}, {TILE_ILV_64x64_2CU, 2}},
      {"mimi.ff1", {TILE_ILV_64x64_2CU, 1}, {TILE_ILV_64x64_2CU, 1}},
      {"mimi.ff2", {TILE_ILV_64x64_2CU, 4}, {TILE_ILV_64x64_2CU, 2}},
      {"seanet.conv0", {TILE_ILV_64x64_2CU, 4}, {TILE_ILV_64x64_2CU, 2}},
      {"seanet.up0.convtr", {TILE_ILV_64x64_2CU, 4}, {TILE_ILV_64x64_2CU, 2}},
      {"seanet.up1.convtr", {TILE_ILV_64x64_2CU, 1}, {TILE_ILV_64x64_2CU, 1}},
      {"seanet.up2.convtr", {TILE_ILV_64x64_2CU, 1}, {TILE_ILV_64x64_2CU, 1}},
      // the stage-0/1 residual convs when not fused (see resblock_fused)
      {"seanet.up0.res_conv3", {TILE_RB_32x64, 1}, {TILE_RB_32x64, 1}},
      {"seanet.up1.res_conv3", {TILE_RB_64x64, 1}, {TILE_RB_64x64, 1}},
      {"seanet.up0.res_conv1", {TILE_GLDS_64x64, 1}, {TILE_GLDS_64x64, 1}},
      {"seanet.up1.res_conv1", {TILE_GLDS_64x64, 1}, {TILE_GLDS_64x64, 1}},
      {"seanet.up2.res_conv3", {TILE_GLDS_128x32, 1}, {TILE_GLDS_128x32, 1}},
      {"seanet.up2.res_conv1", {TILE_GLDS_64x64, 1}, {TILE_GLDS_RB_128x64, 1}},
  };
  for (const auto& t : table)
    if (op == t.op) return pipeline ? t.pipe : t.seq;
  throw Error(PTTS_ERR_INVALID, "no tile for " + op);
}
// The back part's tile under back_mfma bf16 / bf16x6: the operand twin of the ILV tile the f32 table
// names. Policy, not existence: bf16 keeps 128 x 64 and 128 x 128 (2 per CU), bf16x6 only 128 x 64;
// every other tile of the f32 table (register-blocked, non-ILV) maps to the 64 x 64 twin.
static int back_twin(int layout, int back_mfma) {
  if (back_mfma == PTTS_BACK_BF16)
    return TILE_TWIN_BF16 +
           (layout == TILE_ILV_128x64_2CU || layout == TILE_ILV_128x128_2CU ? layout : TILE_ILV_64x64_2CU);
  if (back_mfma == PTTS_BACK_F32X6)
    return TILE_TWIN_BF16X6 + (layout == TILE_ILV_128x64_2CU ? layout : TILE_ILV_64x64_2CU);
  return layout;
}

// The engine's own pass over the frames the front parts left in buffers hb .. hb + nfr - 1
Engine::BackPass Engine::step_pass(int hb, int nfr) const {
  BackPass p;
  p.nfr = nfr;
  for (int f = 0; f < nfr; ++f) {
    p.lat[f] = lat_out_[(hb + f) % nhb_];
    p.flags[f] = flags_[(hb + f) % nhb_];
  }
  p.pcm = nfr_ == 1 ? pcm_[hb] : pcmp_[hb / nfr_];
  p.pcm_ld = (long)nfr_ * FRAME;
  p.wire = wire_ ? wireb_[nfr_ > 1 ? hb / nfr_ : hb] : nullptr;
  return p;
}

// BACK part of a step: Mimi decode of the rows [0, B) of the pass's frames, over the workspace and
// codec state bb.
void Engine::build_back(std::vector<Op>& ops, int B, const BackBufs& bb, const BackPass& pass) {
  const int nfr = pass.nfr, pcm_frames = (int)(pass.pcm_ld / FRAME);
  PTTS_REQUIRE(nfr >= 1 && nfr <= nfr_, "frames per back pass out of range");
  PTTS_REQUIRE(pcm_frames >= nfr, "pass block smaller than the pass");
  // (the launch arguments hold NFR_MAX frames: those past the pass repeat its last)
  std::array<const float*, NFR_MAX> lat;
  std::array<const FrameFlags*, NFR_MAX> fl;
  for (int f = 0; f < NFR_MAX; ++f) {
    lat[f] = pass.lat[std::min(f, nfr - 1)];
    fl[f] = pass.flags[std::min(f, nfr - 1)];
  }
  const bool big = B >= 16;  // B * 16 >= 256 Mimi rows: the LDS-DMA tiles fill the chip
  auto tile = [&](const std::string& op, int small_splits) {
    BackTile t = big ? back_tile(op, pipeline_) : BackTile{TILE_KSPLIT_4W, small_splits};
    // four-frame passes: SEANet conv0 and the stage-0 transposed conv have twice a pair pass's rows
    // (B * 64: 256 / 1,024 64 x 64 tiles at B = 32), enough to fill the chip unsplit, so neither
    // writes slabs nor needs its reduce launch (steady step 0.5179 -> 0.5137 ms,
    // profiles/r06/ab_quad_splits.txt; unsplit in pair passes: +2.7 %, profiles/r06/ab1.txt)
    if (big && nfr >= 4 && (op == "seanet.conv0" || op == "seanet.up0.convtr")) t.splits = 1;
    if (big) t.layout = back_twin(t.layout, back_mfma_);
    tile_override(op, t.layout, t.splits);  // probe builds only (tools/back_tune.py)
    return t;
  };
  // ---- Mimi decode (mimi.rs:143-157): quantize + upsample, decoder transformer, SEANet decoder
  {
    const float *sd = W(L_.emb_std), *mn = W(L_.emb_mean), *wq = W(L_.quant_w), *wu = W(L_.up_w);
    const float *lw = W(L_.mdec[0].n1w), *lb = W(L_.mdec[0].n1b);
    const float* qin = bb.qprev;
    float* qout = bb.qcur;
    float *x = bb.mx, *h = bb.mh;
    ops.push_back({"mimi.quant_upsample",
                   [=](hipStream_t s) { quant_upsample(lat.data(), fl.data(), nfr, B, sd, mn, wq, wu, qin, qout, x, h, lw, lb, s); },
                   (double)B * nfr * (2.0 * MD * LDIM + 2.0 * MD * 2 * UP + 8.0 * UP * MD),
                   4.0 * ((double)B * nfr * (LDIM + 2 * MD + 2.0 * UP * MD) + 2.0 * MD * LDIM + MD * 2.0 * UP + 2.0 * MD)});
  }
  const int MR = B * UP * nfr;  // Mimi rows of the pass: 16 per frame per utterance
  RowMap mmap{0, UP * nfr, 0, bb.mpos};
  // a split-K GEMM into the back part's own slab buffer, its epilogue in a row reduce
  auto split_gemm = [&](const std::string& name, const float* X, int M, const float* Wt, int N, int K, BackTile t) {
    PTTS_REQUIRE(t.splits >= 1 && t.splits <= 16, name + ": split-K 1..16");
    PTTS_REQUIRE((size_t)t.splits * M * N <= bb.mpcap, "back split-K slab buffer too small");
    GemmArgs a = dense_gemm(t.layout, M, N, K, X, K, Wt);
    a.S = t.splits;
    a.partial = bb.mpartial;
    attach_split(a);
    const int S = t.splits;
    ops.push_back({name, [a, S](hipStream_t s) { gemm(a, S, s); }, 2.0 * M * N * K,
                   4.0 * ((double)N * K + (double)M * K + (double)S * M * N)});
  };
  for (int l = 0; l < MNL; ++l) {
    const Layout::TL& t = L_.mdec[l];
    const std::string p = "mimi.l" + std::to_string(l);
    KvStore kv{bb.ring + (long)l * ring_layer_, ring_slot_, RING};
    {  // QKV in one pass; RoPE + ring append inside the attention launch
      const BackTile tq = tile("mimi.qkv", 1);
      dense_op(ops, p + ".qkv_gemm", bb.mh, MR, W(t.in_proj), 3 * MD, MD, nullptr, ACT_NONE, nullptr, nullptr, bb.mqkv,
               tq.layout);
      const float* qkv = bb.mqkv;
      float* O = bb.mo;
      // per utterance: the K and V of its window (W keys x 8 heads x 64 x 2, read once for its 16
      // queries), its 16 QKV rows in, the 16 output rows, the appended K/V; 16 queries x W keys x
      // 8 heads x 64 x 4 flops = 65,536 W
      const double Wn = plan_win_ > 0 ? plan_win_ : (double)(MCTX + UP - 1);
      if (nfr == 1) {
        ops.push_back({p + ".attention", [=](hipStream_t s) { attention16_qkv(qkv, MR, MNH, mmap, kv, MCTX, O, s); },
                       (double)B * 65536.0 * Wn,
                       (double)B * (4.0 * 2 * MNH * 64 * Wn + 4.0 * UP * (3.0 * MD + MD + 2.0 * MD))});
      } else {  // two frames: the second frame's queries see the first frame's keys, appended by
        // other workgroups, so the append (with RoPE) is its own launch ahead of the attention
        float* Q = bb.mq;
        ops.push_back({p + ".qkv_rope", [=](hipStream_t s) { qkv_rope_append(nullptr, 0, qkv, MR, MNH, mmap, kv, Q, s); },
                       0.0, 4.0 * MR * (3.0 * MD + 3.0 * MD)});
        ops.push_back({p + ".attention", [=](hipStream_t s) { attention(Q, MR, MNH, mmap, kv, MCTX, O, s); },
                       (double)B * nfr * 65536.0 * Wn,
                       (double)B * nfr * (4.0 * 2 * MNH * 64 * Wn + 4.0 * UP * (MD + MD))});
      }
    }
    {  // out projection, split-K; LayerScale + residual and this layer's norm2 in the reduce
      const BackTile to = tile("mimi.out", 4);
      split_gemm(p + ".out_gemm", bb.mo, MR, W(t.out_proj), MD, MD, to);
      RowReduceArgs r{};
      r.P = bb.mpartial;
      r.S = to.splits;
      r.M = MR;
      r.N = MD;
      r.gate = W(t.ls1);  // per-column LayerScale: gate row stride 0
      r.ldg = 0;
      r.R = bb.mx;
      r.ldr = MD;
      r.Y = bb.mx;
      r.ldy = MD;
      r.ln = 1;
      r.ln_w = W(t.n2w);
      r.ln_b = W(t.n2b);
      r.eps = 1e-5f;
      r.Hout = bb.mh;
      r.ldh = MD;
      ops.push_back(rr_op(p + ".out_reduce_ln2", r));
    }
    {  // linear1 + GELU in the tile epilogue
      const BackTile tf = tile("mimi.ff1", 1);
      dense_op(ops, p + ".ff1_gemm", bb.mh, MR, W(t.l1), MFF, MD, nullptr, ACT_GELU, nullptr, nullptr, bb.mu, tf.layout);
    }
    {  // linear2 (K = 2048), split-K; LayerScale + residual (+ the next layer's norm1) in the reduce.
       // Few rows (B < 16, the first-chunk path): 32x32 tiles, 8 slices (16 -> 128 workgroups)
      const BackTile tf = tile("mimi.ff2", 8);
      split_gemm(p + ".ff2_gemm", bb.mu, MR, W(t.l2), MD, MFF, tf);
      RowReduceArgs r{};
      r.P = bb.mpartial;
      r.S = tf.splits;
      r.M = MR;
      r.N = MD;
      r.gate = W(t.ls2);
      r.ldg = 0;
      r.R = bb.mx;
      r.ldr = MD;
      r.Y = bb.mx;
      r.ldy = MD;
      if (l + 1 < MNL) {  // the next layer's norm1 on the reduced rows (no separate LayerNorm launch)
        r.ln = 1;
        r.ln_w = W(L_.mdec[l + 1].n1w);
        r.ln_b = W(L_.mdec[l + 1].n1b);
        r.eps = 1e-5f;
        r.Hout = bb.mh;
        r.ldh = MD;
      }
      ops.push_back(rr_op(p + ".ff2_reduce", r));
    }
  }
  // SEANetDecoder (seanet.rs:396-402): conv0 -> [ELU, convtr(r), resblock] x3 -> ELU, conv(64->1).
  // Every ELU is applied once, by the producer of the activation (elu_out / the dual store Y2),
  // so the consumers' operand loads are plain: a0, ce and ca hold ELU'd activations (and so do the
  // histories of the convs that read them; elu(0) = 0 keeps the zero reset valid), cb stays raw for
  // the resblock skip. Transposed convs run with their r phases merged into N: one 2-tap conv over
  // rows (x[q-1], x[q]) whose output row q is the r time rows q*r .. q*r+r-1 of the channels-last
  // output, N = r * Cout (packed [r][Cout][2][Cin] = [r*Cout][2*Cin]).
  {  // conv0 (K = 7 x 512, M = 16 B rows): split-K fills the chip; bias + ELU in the reduce (every B:
     // at B = 1 the unsplit launch had 16 workgroups, 27.4 us)
    const BackTile tc = tile("seanet.conv0", 8);
    if (big && tc.splits == 1) {  // unsplit: bias + ELU in the tile epilogue, no reduce launch
      conv_op(ops, "seanet.conv0", bb.mx, B, 16 * nfr, 512, bb.hist[0], 6, 1, 0, W(L_.dc0_w), 512, 7, 1, W(L_.dc0_b),
              nullptr, bb.a0, 16 * nfr, 1, tc.layout, 1, nullptr, 1);
    } else {
    const int s_c0 = std::max(tc.splits, 2);
    conv_op(ops, "seanet.conv0", bb.mx, B, 16 * nfr, 512, bb.hist[0], 6, 1, 0, W(L_.dc0_w), 512, 7, 1, nullptr, nullptr,
            nullptr, 16 * nfr, 1, big ? tc.layout : TILE_GLDS_64x64, 0, nullptr, s_c0, bb.mpartial, bb.mpcap);
    RowReduceArgs r{};
    r.P = bb.mpartial;
    r.S = s_c0;
    r.M = B * 16 * nfr;
    r.N = 512;
    r.bias = W(L_.dc0_b);
    r.act = ACT_ELU;
    r.Y = bb.a0;
    r.ldy = 512;
    ops.push_back(rr_op("seanet.conv0_reduce", r));
    }
  }
  const float* cin_buf = bb.a0;
  int T = 16 * nfr, ch = 512;
  // a pass's PCM is [B][pcm_frames][1920] in its pass block (frames past nfr untouched)
  float* pcm_out = pass.pcm;
  const long pcm_ld = pass.pcm_ld;
  bool fin_fused = false;  // the final conv ran in the stage-2 residual block's epilogue
  // fused residual blocks (k3 conv + ELU + k1 conv + skip + ELU, the hidden rows in LDS) where they
  // beat the two conv launches: stage 2 (480 workgroups; 22.5 us against 16.8 + 11.0). Stages
  // 0 and 1 have 96 / 160 workgroups of it and measured slower than their two tuned launches.
  // PTTS_RESBLOCK_STAGES (probe builds): bit mask of the stages that fuse.
  // Four-frame passes give stages 0 and 1 four times their single-frame workgroups (384 / 640 at
  // B = 32), and there the fused block of every stage pays: 0.5049 -> 0.5008 ms
  // (profiles/r06/ab_resblock.txt; stage 1 fused in pair passes: +0.8 %, round 5)
  int fused_stages = nfr >= 4 ? 7 : 4;
  if (probe_env("PTTS_RESBLOCK_STAGES")) fused_stages = atoi(probe_env("PTTS_RESBLOCK_STAGES"));
  // (f32 only: its own MFMA loop). A fused stage's (unsplit) transposed conv stores no ELU'd copy:
  // the block ELUs the raw rows as they enter LDS
  auto fuse_res = [&](int i) { return big && (fused_stages >> i & 1) && back_mfma_ == PTTS_BACK_F32; };
  // stages whose fused residual block reads the RAW transposed-conv rows (E = elu(R) applied as the
  // rows enter LDS): every fused stage whose transposed conv is unsplit (a split one's reduce stores
  // both the raw and the ELU'd rows)
  bool raw_only[3] = {false, false, false};
  for (int i = 0; i < 3; ++i) {
    const int r = RATIOS[i];
    const std::string p = "seanet.up" + std::to_string(i);
    const BackTile tt = tile(p + ".convtr", 1);
    raw_only[i] = fuse_res(i) && !(big && tt.splits > 1);
    if (big && tt.splits > 1) {  // stage 0 (M = 16 B rows): split-K; bias + dual raw / ELU store in the reduce
      PTTS_REQUIRE(i == 0, "split-K transposed conv: stage 0 only");
      conv_op(ops, p + ".convtr", cin_buf, B, T, ch, bb.hist[1], 1, 1, 0, W(L_.dtr_w[0]), r * (ch / 2), 2, 1, nullptr,
              nullptr, nullptr, T, 1, tt.layout, 0, nullptr, tt.splits, bb.mpartial, bb.mpcap);
      RowReduceArgs rr{};
      rr.P = bb.mpartial;
      rr.S = tt.splits;
      rr.M = B * T;
      rr.N = r * (ch / 2);
      rr.bias = trb_[0];
      rr.Y = bb.cb[0];
      rr.Y2 = bb.ce[0];
      rr.ldy = r * (ch / 2);
      ops.push_back(rr_op(p + ".convtr_reduce", rr));
    } else {
      // stage 2 fused below: no ELU'd copy (the residual block ELUs the raw rows as it loads them)
      conv_op(ops, p + ".convtr", cin_buf, B, T, ch, bb.hist[1 + 2 * i], 1, 1, 0, W(L_.dtr_w[i]), r * (ch / 2), 2, 1,
              trb_[i], nullptr, bb.cb[i], T, 1, tt.layout, 0, fuse_res(i) ? nullptr : bb.ce[i]);
    }
    T *= r;
    ch /= 2;
    if (fuse_res(i)) {
      ResBlockArgs rb{bb.ce[i], bb.hist[2 + 2 * i], bb.cb[i], W(L_.dra_w[i]), W(L_.dra_b[i]), W(L_.drb_w[i]),
                      W(L_.drb_b[i]), bb.ca[i], B, T, ch};
      const double hd = ch / 2;
      double fl = 2.0 * B * T * (hd * 3 * ch + ch * hd);
      double by = 4.0 * ((double)B * T * ch * 3 + B * 2.0 * ch + hd * 3 * ch + ch * hd + hd + ch);
      if (raw_only[i]) {  // E = elu(R) as the rows enter LDS (a split-K reduce stores both)
        rb.E = bb.cb[i];
        rb.e_raw = 1;
        by -= 4.0 * B * T * ch;  // E and R are the same rows: read once
      }
      if (i == 2 && T % RESBLOCK_FIN_TT == 0) {  // + the final conv (64 -> 1, k = 3) of the tile's rows
        rb.fw = W(L_.dfin_w);
        rb.fb = W(L_.dfin_b);
        rb.fH = bb.hist[7];
        rb.fout = pcm_out;
        rb.fld = pcm_ld;
        rb.fside = bb.fin_side;
        fin_fused = true;
        fl += 2.0 * B * T * 3 * 64;
        by += 4.0 * ((double)B * T + B * 2.0 * 64 + 3 * 64 + 1);
      }
      ops.push_back({p + ".resblock", [rb](hipStream_t s) { resblock(rb, s); }, fl, by});
    } else {  // the two convs (few rows: 32x32 tiles, more workgroups than the fused tiles)
      const int lr3 = big ? tile(p + ".res_conv3", 1).layout : TILE_KSPLIT_4W,
                lr1 = big ? tile(p + ".res_conv1", 1).layout : TILE_KSPLIT_4W;
      conv_op(ops, p + ".res_conv3", bb.ce[i], B, T, ch, bb.hist[2 + 2 * i], 2, 1, 0, W(L_.dra_w[i]), ch / 2, 3, 1,
              W(L_.dra_b[i]), nullptr, bb.cv[i], T, 1, lr3, 1);
      conv_op(ops, p + ".res_conv1", bb.cv[i], B, T, ch / 2, nullptr, 0, 1, 0, W(L_.drb_w[i]), ch, 1, 1,
              W(L_.drb_b[i]), bb.cb[i], bb.ca[i], T, 1, lr1, 1);
    }
    cin_buf = bb.ca[i];
  }
  if (!fin_fused) {
    const float *X = bb.ca[2], *H = bb.hist[7], *w = W(L_.dfin_w), *b = W(L_.dfin_b);
    float* Y = pcm_out;
    const int TF = FRAME * nfr;
    ops.push_back({"seanet.conv_final", [=](hipStream_t s) { conv_cout1(X, H, B, TF, 64, 3, w, b, Y, 0, s, pcm_ld); },
                   2.0 * B * TF * 3 * 64, 4.0 * ((double)B * TF * 64 + B * 2.0 * 64 + B * TF + 3 * 64 + 1)});
  }
  // ---- commit of the back part: conv histories and Mimi positions of rows with a frame (it also
  // adds the fused final conv's tile-boundary shares into the PCM)
  PTTS_REQUIRE(pass.commit || !fin_fused, "a pass without the commit: the small-row path only");
  if (pass.commit) {
    CommitArgs c{};
    const float* srcs[8] = {bb.mx, bb.a0, bb.ce[0], bb.ca[0], bb.ce[1], bb.ca[1], bb.ce[2], bb.ca[2]};
    for (int i = 0; i < 8; ++i) c.h[i] = HistDesc{srcs[i], bb.hist[i], hist_T_[i] * nfr, hist_C_[i], hist_P_[i]};
    for (int i = 0; i < 3; ++i)  // a raw-only fused stage's k3-conv history: elu(raw rows)
      if (raw_only[i]) c.h[2 + 2 * i] = HistDesc{bb.cb[i], bb.hist[2 + 2 * i], hist_T_[2 + 2 * i] * nfr, hist_C_[2 + 2 * i], hist_P_[2 + 2 * i], 1};
    c.nh = 8;
    c.B = B;
    for (int f = 0; f < NFR_MAX; ++f) c.flags[f] = fl[f];
    c.nfr = nfr;
    c.mpos = bb.mpos;
    c.qcur = bb.qcur;
    c.qprev = bb.qprev;
    if (fin_fused) {
      c.fin_pcm = pcm_out;
      c.fin_side = bb.fin_side;
      c.fin_T = FRAME * nfr;
      c.fin_ld = pcm_ld;
    }
    double hb_bytes = 0;  // every history row is read from its activation and stored
    for (int i = 0; i < 8; ++i) hb_bytes += 8.0 * B * hist_P_[i] * hist_C_[i];
    ops.push_back({"commit", [c](hipStream_t s) { step_commit(c, s); }, 0.0, hb_bytes + 16.0 * B});
  }
  // ---- wire stage (wire-enabled engines): after the commit, which still adds the fused final
  // conv's tile-boundary shares into the PCM
  if (pass.wire) {
    if (tempo_) {  // the speed rows' chunks first: the wire stage reads them in place of the PCM
      TempoArgs ta{};
      ta.B = B;
      ta.nfr = nfr;
      ta.pcm_frames = pcm_frames;
      ta.out_frames = nfr_;
      ta.pcm = pcm_out;
      for (int f = 0; f < NFR_MAX; ++f) ta.flags[f] = fl[f];
      ta.sp = tempo_sp_;
      ta.state = tempo_state_;
      ta.hist = tempo_hist_;
      ta.win = tempo_win_;
      ta.out = tempo_out_;
      ta.counts = tempo_cnt_;
      ops.push_back({"tempo", [ta](hipStream_t s) { tempo_stage(ta, s); }, 0.0,
                     (double)B * nfr * 4.0 * (FRAME + TEMPO_OUT_MAX)});
    }
    if (pitch_) {  // then the pitch rows' chunks, from the PCM or the tempo chunks (section 23)
      PitchArgs pa{};
      pa.B = B;
      pa.nfr = nfr;
      pa.pcm_frames = pcm_frames;
      pa.out_frames = nfr_;
      pa.pcm = pcm_out;
      for (int f = 0; f < NFR_MAX; ++f) pa.flags[f] = fl[f];
      pa.step = pitch_step_;
      pa.tempo_sp = tempo_sp_;
      pa.tin = tempo_out_;
      pa.tcnt = tempo_cnt_;
      pa.state = pitch_state_;
      pa.hist = pitch_hist_;
      pa.tab = pitch_tab_;
      pa.out = pitch_out_;
      pa.counts = pitch_cnt_;
      ops.push_back({"pitch", [pa](hipStream_t s) { pitch_stage(pa, s); }, 0.0,
                     (double)B * nfr * 4.0 * (TEMPO_OUT_MAX + PITCH_OUT_MAX)});
    }
    if (level_) {  // then the level rows' chunks, from whatever the wire stage would read (section 24)
      LevelArgs la{};
      la.B = B;
      la.nfr = nfr;
      la.pcm_frames = pcm_frames;
      la.out_frames = nfr_;
      la.pcm = pcm_out;
      for (int f = 0; f < NFR_MAX; ++f) la.flags[f] = fl[f];
      la.gain = level_gain_;
      la.ceiling = level_ceiling_;
      if (tempo_) {
        la.tempo_sp = tempo_sp_;
        la.tin = tempo_out_;
        la.tcnt = tempo_cnt_;
      }
      if (pitch_) {
        la.pitch_step = pitch_step_;
        la.pin = pitch_out_;
        la.pcnt = pitch_cnt_;
      }
      la.state = level_state_;
      la.hist = level_hist_;
      la.out = level_out_;
      la.counts = level_cnt_;
      ops.push_back({"level", [la](hipStream_t s) { level_stage(la, s); }, 0.0,
                     (double)B * nfr * 4.0 * (PITCH_OUT_MAX + LEVEL_OUT_MAX)});
    }
    WireArgs w{};
    w.B = B;
    w.nfr = nfr;
    w.pcm_frames = pcm_frames;
    w.out_frames = nfr_;
    w.pcm = pcm_out;
    for (int f = 0; f < NFR_MAX; ++f) w.flags[f] = fl[f];
    w.fmt = wire_fmt_;
    w.frames = wire_frames_;
    w.tail = wire_tail_;
    w.taps = wire_taps_;
    for (int r = 0; r < WIRE_RATES; ++r) w.plan[r] = wire_plan_[r];
    w.counts = (int*)pass.wire;
    w.out = pass.wire + wire_head_bytes();
    w.chunk = wire_chunk_max();
    if (tempo_) {
      w.tempo_sp = tempo_sp_;
      w.tin = tempo_out_;
      w.tcnt = tempo_cnt_;
    }
    if (pitch_) {
      w.pitch_step = pitch_step_;
      w.pin = pitch_out_;
      w.pcnt = pitch_cnt_;
    }
    if (level_) {
      w.level_gain = level_gain_;
      w.lin = level_out_;
      w.lcnt = level_cnt_;
    }
    if (flac_) w.first = flac_first_;
    if (loud_) {  // the metered rows' sub-block energies, from what the wire stage reads (section 27)
      LoudArgs lo{};
      lo.B = B;
      lo.nfr = nfr;
      lo.pcm_frames = pcm_frames;
      lo.out_frames = nfr_;
      lo.pcm = pcm_out;
      for (int f = 0; f < NFR_MAX; ++f) lo.flags[f] = fl[f];
      lo.tempo_sp = w.tempo_sp, lo.tin = w.tin, lo.tcnt = w.tcnt;
      lo.pitch_step = w.pitch_step, lo.pin = w.pin, lo.pcnt = w.pcnt;
      lo.level_gain = w.level_gain, lo.lin = w.lin, lo.lcnt = w.lcnt;
      lo.state = loud_state_;
      lo.pend = loud_pend_;
      lo.filt = loud_filt_;
      lo.out = (LoudRecord*)(pass.wire + wire_loud_off());
      lo.k = loud_coef_;
      ops.push_back({"loud", [lo](hipStream_t s) { loud_stage(lo, s); }, 0.0, (double)B * nfr * 4.0 * LOUD_IN_MAX});
    }
    ops.push_back({"wire", [w](hipStream_t s) { wire_stage(w, s); }, 0.0,
                   (double)B * nfr * (4.0 * FRAME + wire_chunk_max())});
    if (flac_) {  // the FLAC rows' 16-bit chunks become frames, in place (section 21)
      FlacArgs fa{};
      fa.B = B;
      fa.out_frames = nfr_;
      fa.fmt = wire_fmt_;
      fa.first = flac_first_;
      fa.out = w.out;
      fa.counts = w.counts;
      fa.chunk = w.chunk;
      fa.nframes = w.counts + (size_t)max_slots_ * nfr_;  // the block's head: counts | frame counts | index
      fa.index = fa.nframes + (size_t)max_slots_ * nfr_;
      Op op{"flac", [fa](hipStream_t s) { flac_stage(fa, s); }, 0.0, (double)B * nfr * 2.0 * wire_chunk_max()};
      // an isolated replay (time_op) encodes fresh 16-bit chunks: the stage overwrites its input
      op.prep = [w](hipStream_t s) { wire_stage(w, s); };
      ops.push_back(op);
    }
  }
}

// The whole step in plan order (front then back, buffer 0): plan listing and per-op timing.
std::vector<Op> Engine::build_step(int B) {
  std::vector<Op> ops;
  build_front(ops, B, 0, lsd_run_for(B));
  build_back(ops, B, bbm_, step_pass(0, nfr_));
  return ops;
}

std::vector<std::string> Engine::plan_names(int B) {
  PTTS_REQUIRE(B >= 1 && B <= max_slots_, "n_rows out of range");
  // the attention costs are for the rows' current positions (what time_op replays): the mean
  // FlowLM context over rows [0, B) and the mean Mimi window (positions + 16 queries, <= 265)
  sync();
  std::vector<int> fp(B), mp(B);
  PTTS_HIP(hipMemcpy(fp.data(), fpos_, sizeof(int) * B, hipMemcpyDeviceToHost));
  PTTS_HIP(hipMemcpy(mp.data(), bbm_.mpos, sizeof(int) * B, hipMemcpyDeviceToHost));
  double L = 0, Wn = 0, kvu = 0;
  std::vector<const float*> seen;  // distinct shared voice prefixes: read once per launch
  for (int b = 0; b < B; ++b) {
    L += fp[b] + 1;
    Wn += std::min(mp[b] + UP, MCTX + UP - 1);
    const int F = share_voice_ && h_vpre_[b] ? h_vlen_[b] : 0;
    kvu += fp[b] + 1 - F;
    if (F > 0 && std::find(seen.begin(), seen.end(), h_vpre_[b]) == seen.end()) {
      seen.push_back(h_vpre_[b]);
      kvu += F;
    }
  }
  plan_ctx_ = L / B;
  plan_win_ = Wn / B;
  plan_kvu_ = kvu;
  std::vector<std::string> v;
  char buf[64];
  for (auto& op : build_step(B)) {
    snprintf(buf, sizeof buf, "\t%.6g\t%.6g", op.flops, op.bytes);
    v.push_back(op.name + buf);
  }
  return v;
}

// A stream wait costs the front stream a few us at the graph boundary even on a completed event
// (profiles/r04/graph_boundary_ab.txt): the hand-off buffer waits are enqueued only when the host
// sees the event still pending (the pass that last read the buffer is three passes old, so it has
// normally completed by the time the call is issued).
void Engine::wait_unless_done(hipStream_t s, hipEvent_t e) {
  const hipError_t r = hipEventQuery(e);
  if (r == hipSuccess) return;
  (void)hipGetLastError();
  PTTS_HIP(hipStreamWaitEvent(s, e, 0));
}

// The frame(s) a back part decoded leave HBM by a copy enqueued right after its graph on the same
// stream (fetch() reads host memory): a DMA-engine transfer, not a blit-kernel node of the graph,
// whose workgroups held CUs beside the front part while the host writes drained.
void Engine::copy_out(int B, int hb, hipStream_t s) {
  if (nfr_ > 1) {  // every frame of the pass (PCM and meta) in one copy
    const size_t n = (size_t)max_slots_ * nfr_ * FRAME + nfr_ * ((meta_floats_ + 31) / 32 * 32);
    PTTS_HIP(hipMemcpyAsync(h_pcmp_[hb / nfr_], pcmp_[hb / nfr_], sizeof(float) * n, hipMemcpyDeviceToHost, s));
  } else {
    PTTS_HIP(hipMemcpyAsync(h_pcm_[hb], pcm_[hb], sizeof(float) * B * FRAME, hipMemcpyDeviceToHost, s));
    PTTS_HIP(hipMemcpyAsync(h_meta_[hb], meta_[hb], sizeof(float) * meta_floats_, hipMemcpyDeviceToHost, s));
  }
  if (wire_) {  // the pass's byte counts, and the chunk slots of its rows when one of them has a format
    const int p = nfr_ > 1 ? hb / nfr_ : hb;
    bool any = false;  // (a slot's format changes only at its admission, whose reset drops its pending frames)
    for (int b = 0; b < B; ++b) any = any || slot_wire_[b];
    PTTS_HIP(hipMemcpyAsync(h_wireb_[p], wireb_[p], any ? wire_block_bytes(B) : wire_head_bytes(),
                            hipMemcpyDeviceToHost, s));
  }
  if (align_) {  // the alignment blocks of the pass's buffers, when a row of their front parts was in the stage
    bool any = false;
    for (int f = 0; f < nfr_; ++f) any = any || align_any_[hb + f];
    if (any) {
      const size_t off = (size_t)hb * max_slots_ * ALIGN_ROW, n = (size_t)nfr_ * max_slots_ * ALIGN_ROW;
      PTTS_HIP(hipMemcpyAsync(h_alignb_ + off, alignb_ + off, sizeof(float) * n, hipMemcpyDeviceToHost, s));
    }
  }
}

hipGraphExec_t Engine::part_graph(int part, int B, int hb, int qp, int nfr, int lsd_run) {
  if (part == 0) qp = nfr = 0;  // the front part does not use the quantizer history
  else lsd_run = 0;             // nor the back part the Euler step count
  const int key = ((((B * 2 + part) * NHB + hb) * 2 + qp) * (NFR_MAX + 1) + nfr) * (LSD_MAX + 1) + lsd_run;
  auto it = graphs_.find(key);
  if (it != graphs_.end()) return it->second;
  std::vector<Op> ops;
  if (part == 0) build_front(ops, B, hb, lsd_run);
  else build_back(ops, B, bbm_, step_pass(hb, nfr));
  hipGraph_t g = nullptr;
  // captured on the stream it is launched on (the back part of a pipelined step: stream_be_)
  hipStream_t cs = part == 1 && pipeline_ ? stream_be_ : stream_;
  PTTS_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
  // back part of a pipelined step: its launches leave room for the concurrent front part
  set_wg_cap(part == 1 && pipeline_ ? back_cap_ : 0);
  // the back part's tile waves issue at priority 3 beside the front part's (pair passes: steady step
  // 0.5533 -> 0.5496 ms, devfn.h back_prio), except in four-frame passes, whose back part has four
  // steps' time per pass: there the front part's waves keep the default order (0.5134 -> 0.5106
  // ms, profiles/r06/ab_bf8.txt)
  set_back_hi(part == 1 && pipeline_ && nfr_ >= 4 ? 0 : 1);
  // per-op cap override for back-part launches: PTTS_OP_CAP="name=cap,..." (tuning)
  const char* opcap = part == 1 && pipeline_ ? probe_env("PTTS_OP_CAP") : nullptr;
  try {
#ifdef PTTS_PROBES
    if (stamp_ring_) stamp(stamp_ring_, stamp_ctr_, (unsigned)(part << 8 | hb << 1), cs);
#endif
#ifdef PTTS_PROBES
    // PTTS_STAMP_OPS: a stamp ahead of every op as well (two back to back first: the stamp cost)
    const bool op_stamps = stamp_ring_ && probe_env("PTTS_STAMP_OPS");
    if (op_stamps) {
      stamp(stamp_ring_, stamp_ctr_, 0x10000u | part << 12 | 0xFFEu, cs);
      stamp(stamp_ring_, stamp_ctr_, 0x10000u | part << 12 | 0xFFFu, cs);
      stamp_names_[part].clear();
      for (const Op& op : ops) stamp_names_[part].push_back(op.name);
    }
    unsigned op_i = 0;
#endif
    for (const Op& op : ops) {
#ifdef PTTS_PROBES
      if (op_stamps) stamp(stamp_ring_, stamp_ctr_, 0x10000u | part << 12 | op_i++, cs);
#endif
      if (opcap) {
        int cap = back_cap_;
        const std::string e(opcap), key = op.name + "=";
        const size_t at = e.find(key);
        if (at != std::string::npos && (at == 0 || e[at - 1] == ',')) cap = atoi(e.c_str() + at + key.size());
        set_wg_cap(cap);
      }
      op.fn(cs);
    }
    // part 0: the hand-off timeout word (read by fetch() without a device round trip) and the
    // flags of rows past B are front_commit's side jobs; part 1: the frames leave HBM by copy_out()
    // after the graph (no copy nodes in either graph)
#ifdef PTTS_PROBES
    if (stamp_ring_) stamp(stamp_ring_, stamp_ctr_, (unsigned)(part << 8 | hb << 1 | 1), cs);
#endif
  } catch (...) {
    set_wg_cap(0);
    set_back_hi(1);
    (void)hipStreamEndCapture(cs, &g);
    throw;
  }
  set_wg_cap(0);
  set_back_hi(1);
  PTTS_HIP(hipStreamEndCapture(cs, &g));
  hipGraphExec_t ge = nullptr;
  PTTS_HIP(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
  graph_defs_[key] = g;
  graphs_[key] = ge;
  return ge;
}

// One call = one step of the generation loop for rows [0, B).
//   sequential: front(k) then back(k) on one stream; the call's frame is frame k.
//   pipelined:  front(k) on stream_ || back(k-1) on stream_be_ (the back part decodes the frame
//               the previous call's front part produced); the call's frame is frame k-1. Frame
//               k's hand-off buffer is k % nhb_ (3): front(k)
//               waits only for back(k - nhb_), the last reader of its buffer, and back(k-1) for
//               front(k-1).
void Engine::step_async(int B) {
  PTTS_REQUIRE(B >= 1 && B <= max_slots_, "n_rows out of range");
  call_async(B, true);
}

// A flush call: frames already computed are decoded and delivered as by a step call, but no row
// computes a new frame (every row pauses for the call, as rows past n_rows do). Pipelined engines
// only, and not right after an admission (the admitted rows' first frame must fall on a step
// call: with multi-frame passes it must be the first frame of a pass).
void Engine::flush_async(int B) {
  PTTS_REQUIRE(B >= 1 && B <= max_slots_, "n_rows out of range");
  PTTS_REQUIRE(pipeline_, "flush: pipelined engines only");
  PTTS_REQUIRE(!admitted_since_call_ && act_slots_.empty(), "flush right after an admission: step first");
  call_async(B, false);
}

void Engine::call_async(int B, bool run_front) {
  PTTS_REQUIRE(ready_, "engine weights not finalized");
  PTTS_HIP(hipSetDevice(dev_));
  // Multi-frame passes (nfr = back_frames > 1): one back pass decodes a row's frames of the pass as
  // a prefix (frames nfr j, nfr j + 1, ..). A row the pass's first call did not cover must not
  // produce a later frame of the pass alone, so a call inside a pass covers at most the previous
  // call's rows; rows past that are paused for the call, as rows past n_rows are (a first call
  // that was a flush covered none: the rest of the pass are flushes too).
  if (pipeline_ && nfr_ > 1 && (k_ % nfr_)) {
    B = std::min(B, rows_hb_[(k_ - 1) % nhb_]);
    if (B == 0) run_front = false;
  }
  if (!run_front) B = 0;
  admitted_since_call_ = false;
  prev_hb_ = out_hb_;
  prev_rows_ = out_rows_;
  prev_k_ = out_k_;
  if (!cancel_wins_.empty())  // windows wholly before the oldest frame a fetch can still return
    cancel_wins_.erase(std::remove_if(cancel_wins_.begin(), cancel_wins_.end(),
                                      [this](const CancelWin& w) { return w.to <= prev_k_; }),
                       cancel_wins_.end());
  const int hb = (int)(k_ % nhb_), qp = (int)(k_ & 1);
  // the front part of this call, or (a flush) its hand-off buffer marked frame-less
  // its Euler step count: the largest count among the call's rows that are still open
  const int lsd_run = B > 0 ? lsd_run_for(B) : 0;
  if (B > 0) lsd_last_run_ = lsd_run;
  if (align_) {  // the table as this front part will read it (admissions and cancels are stream-ordered)
    align_any_[hb] = false;
    for (int b = 0; b < B; ++b) align_any_[hb] = align_any_[hb] || slot_align_[b] > 0;
  }
  hipGraphExec_t front = B > 0 ? part_graph(0, B, hb, 0, 0, lsd_run) : nullptr;
  auto run_front_part = [&]() {
    if (pv_read_pending_[hb]) {  // a preview still gathers from this hand-off buffer
      PTTS_HIP(hipStreamWaitEvent(stream_, ev_pv_read_[hb], 0));
      pv_read_pending_[hb] = false;
    }
    if (front && xh_dirty_) refresh_xh();
    if (front) PTTS_HIP(hipGraphLaunch(front, stream_));
    else PTTS_HIP(hipMemsetAsync(flags_[hb], 0, sizeof(FrameFlags) * max_slots_, stream_));
    if (call_ev_from_ >= 0) PTTS_HIP(hipEventRecord(ev_call_[k_ % 4], stream_));
  };
  if (!pipeline_) {
    hipGraphExec_t back = part_graph(1, B, hb, qp, 1);
    run_front_part();
    PTTS_HIP(hipGraphLaunch(back, stream_));
    copy_out(B, hb, stream_);
    out_hb_ = hb;
    out_rows_ = B;
    out_k_ = k_;
  } else if (nfr_ > 1) {
    // Multi-frame passes (nfr = 2 or 4): call k runs front(k) into buffer k % (3 nfr); at k % nfr
    // == 0, k >= nfr, one back pass decodes frames k-nfr .. k-1 (buffers (k-nfr) % (3 nfr) ..) on
    // stream_be_, concurrently with the next fronts. Front(k) waits only for the pass over frame
    // k - 3 nfr, the last reader of its buffer. The call's frame is k - (2 nfr - 1) (its pass was
    // launched by an earlier call; fetch() waits for it).
    const int nf = nfr_, kr = (int)(k_ % nf);
    rows_hb_[hb] = B;
    if (!act_slots_.empty() && kr == 0) {  // rows admitted inside a pass start now
      for (size_t i = 0; i < act_slots_.size(); ++i)
        PTTS_HIP(hipMemcpyAsync(st_ + act_slots_[i], h_act_ + act_slots_[i], sizeof(SlotState), hipMemcpyHostToDevice,
                                stream_));
      PTTS_HIP(hipEventRecord(ev_act_, stream_));
      act_slots_.clear();
    }
    // front(k) overwrites hand-off buffer k % (3 nfr), last read by the pass over frames k - 3 nfr
    // .. k - 2 nfr - 1; the pass's first call waits for that pass, which also read the buffers of
    // the pass's other calls, so they need no wait of their own (stream order). A stream wait
    // costs the front stream ≈ 5 us at the graph boundary even on a completed event (graph
    // stamps, profiles/r04/graph_boundary_ab.txt).
    if (kr == 0) wait_unless_done(stream_, ev_back_[hb]);
    run_front_part();
    launch_previews(B, hb);
    // only the pass's last front part is waited for (by the pass, below)
    if (kr == nf - 1) PTTS_HIP(hipEventRecord(ev_front_[hb], stream_));
    if (kr == 0 && k_ >= nf) {
      const int h0 = (int)((k_ - nf) % nhb_), pq = (int)(((k_ - nf) / nf) & 1);
      // rows: the largest row count of the pass's calls (the first: a call inside a pass covers at
      // most the previous call's rows); nfe: the calls that started frames (the rest were flushes,
      // e.g. a job's drain), the only frames the pass decodes
      int rows = 0, nfe = 0;
      for (int f = 0; f < nf; ++f) {
        const int r = rows_hb_[(h0 + f) % nhb_];
        rows = std::max(rows, r);
        if (r > 0 && nfe == f) nfe = f + 1;
      }
      if (rows > 0) {  // no pass when every call of the pass was a flush
        hipGraphExec_t back = part_graph(1, rows, h0, pq, nfe);
        PTTS_HIP(hipStreamWaitEvent(stream_be_, ev_front_[(h0 + nf - 1) % nhb_], 0));
        if (admit_pending_) {
          PTTS_HIP(hipStreamWaitEvent(stream_be_, ev_admit_, 0));
          admit_pending_ = false;
        }
        PTTS_HIP(hipGraphLaunch(back, stream_be_));
        copy_out(rows, h0, stream_be_);
      }
      PTTS_HIP(hipEventRecord(ev_back_[h0], stream_be_));  // the pass over buffers h0 .. (fetch waits)
    }
    const int lag = 2 * nf - 1;
    out_hb_ = (int)((k_ + nhb_ - lag) % nhb_);
    out_rows_ = k_ >= lag ? rows_hb_[out_hb_] : 0;
    out_k_ = k_ - lag;
  } else {
    const int prev_rows = k_ > 0 ? front_rows_ : B;  // 0: the previous call was a flush
    const int hb1 = (hb + nhb_ - 1) % nhb_, qp1 = qp ^ 1;  // frame k-1
    wait_unless_done(stream_, ev_back_[hb]);
    run_front_part();
    launch_previews(B, hb);
    PTTS_HIP(hipEventRecord(ev_front_[hb], stream_));
    if (prev_rows > 0) {
      hipGraphExec_t back = part_graph(1, prev_rows, hb1, qp1, 1);
      PTTS_HIP(hipStreamWaitEvent(stream_be_, ev_front_[hb1], 0));
      if (admit_pending_) {  // slot state rewritten since the front part this back part decodes
        PTTS_HIP(hipStreamWaitEvent(stream_be_, ev_admit_, 0));
        admit_pending_ = false;
      }
      PTTS_HIP(hipGraphLaunch(back, stream_be_));
      copy_out(prev_rows, hb1, stream_be_);
    }
    PTTS_HIP(hipEventRecord(ev_back_[hb1], stream_be_));
    out_hb_ = hb1;
    out_rows_ = prev_rows;
    out_k_ = k_ - 1;
  }
  front_rows_ = B;
  ++k_;
}

void Engine::sync() {
  PTTS_HIP(hipSetDevice(dev_));
  PTTS_HIP(hipStreamSynchronize(stream_));
  PTTS_HIP(hipStreamSynchronize(stream_be_));
  if (stream_pv_) PTTS_HIP(hipStreamSynchronize(stream_pv_));
}

// Outputs of the last call's frame (see step_async); rows past the rows that frame covered
// report no frame. The step's graphs already copied the frame into pinned host memory.
void Engine::fetch(int B, float* pcm, uint8_t* valid, uint8_t* last, float* eos, float* lat, int calls_back) {
  PTTS_REQUIRE(B >= 1 && B <= max_slots_, "n_rows out of range");
  PTTS_REQUIRE(calls_back == 0 || calls_back == 1, "calls_back must be 0 or 1");
  // the host copies of a call's frame stay intact for two more calls (three hand-off buffers)
  const int q = calls_back ? prev_hb_ : out_hb_;
  const int rows = calls_back ? prev_rows_ : out_rows_;
  const long long fk = calls_back ? prev_k_ : out_k_;  // the call that produced the frame
  // Pipelined: wait only for the back part that produced this call's frame. The front part of
  // the next frame keeps running, so the front stream never idles across calls (the next call's
  // front graph is queued behind it while this one still runs).
  // (multi-frame passes: the pass over buffers nfr p .. records only the event of nfr p)
  if (pipeline_) PTTS_HIP(hipEventSynchronize(ev_back_[q - q % nfr_]));
  else sync();
  const int n = std::min(B, rows);
  if (*h_err_) {  // k_flow_head's bounded hand-off waits: a timeout poisons the frame, fail loudly
    sync();
    *h_err_ = 0;
    PTTS_HIP(hipMemsetAsync(herr_, 0, sizeof(int), stream_));
    // a timed-out launch leaves its hand-off regions part-filled: empty every set again
    if (ffn_hand_) PTTS_HIP(hipMemsetD32Async(ffn_hand_, 0xFFFFFFFFu, 2 * FFN_HAND_FLOATS, stream_));
    PTTS_HIP(hipStreamSynchronize(stream_));
    throw Error(PTTS_ERR_HIP, "persistent launch (FlowLM layers / flow head): an in-launch hand-off wait timed out");
  }
  const float* hl = h_meta_[q];
  const FrameFlags* hf = (const FrameFlags*)(h_meta_[q] + (size_t)max_slots_ * LDIM);
  const float* he = h_meta_[q] + (size_t)max_slots_ * (LDIM + 2);
  // a pass's PCM is [B][nfr][1920] (the frame of buffer q is frame q % nfr)
  auto pcm_row = [&](int b) {
    return nfr_ > 1 ? h_pcmp_[q / nfr_] + ((size_t)b * nfr_ + q % nfr_) * FRAME : h_pcm_[q] + (size_t)b * FRAME;
  };
  for (int b = 0; b < B; ++b) {
    // (a frame of an utterance slots_cancel stopped is not reported: it never drains the slot either)
    const bool ok = b < n && hf[b].valid && (cancel_wins_.empty() || !frame_cancelled(b, fk));
    // its last frame's pass has completed (waited above) - unless the slot was admitted again
    // after that frame's call (a driver that admits the next utterance before fetching the last
    // frame of the previous one, as bench.py does): then the frame is the previous utterance's and
    // the new one's back passes are still to come
    if (ok && hf[b].last && fk >= admit_call_[b]) {
      drained_[b] = codec_ok_[b] = 1;  // (lsd_run_for: the row counts no more)
      // a finished row is still stepped below a higher active slot: out of the align stage, so that
      // k_align stops reading its keys (front-stream order, like the cancel; its delivered frames'
      // rows are in host memory already, and align_any_ of the buffers in flight is set)
      if (align_ && slot_align_[b]) {
        PTTS_HIP(hipMemsetAsync(align_tab_ + b, 0, sizeof(AlignEntry), stream_));
        slot_align_[b] = 0;
      }
    }
    if (valid) valid[b] = ok;
    if (last) last[b] = ok && hf[b].last;
    if (pcm) {
      if (b < n) memcpy(pcm + (size_t)b * FRAME, pcm_row(b), sizeof(float) * FRAME);
      else memset(pcm + (size_t)b * FRAME, 0, sizeof(float) * FRAME);
    }
    if (eos) eos[b] = b < n ? he[b] : 0.f;
    if (lat) {
      if (b < n) memcpy(lat + (size_t)b * LDIM, hl + (size_t)b * LDIM, sizeof(float) * LDIM);
      else memset(lat + (size_t)b * LDIM, 0, sizeof(float) * LDIM);
    }
  }
}

bool Engine::front_done(int calls_back, bool wait) {
  PTTS_REQUIRE(calls_back >= 0 && calls_back <= 3, "calls_back must be in [0, 3]");
  const long long k = k_ - 1 - calls_back;
  if (call_ev_from_ < 0) call_ev_from_ = k_;  // the calls issued from now on record their event
  if (k < 0) return true;
  if (k < call_ev_from_) {  // issued before the first query: no event of its own, the stream's state
    if (wait) {
      PTTS_HIP(hipStreamSynchronize(stream_));
      return true;
    }
    const hipError_t r = hipStreamQuery(stream_);
    if (r == hipErrorNotReady) {
      (void)hipGetLastError();
      return false;
    }
    PTTS_HIP(r);
    return true;
  }
  hipEvent_t e = ev_call_[k % 4];
  if (wait) {
    PTTS_HIP(hipEventSynchronize(e));
    return true;
  }
  const hipError_t r = hipEventQuery(e);
  if (r == hipErrorNotReady) {
    (void)hipGetLastError();
    return false;
  }
  PTTS_HIP(r);
  return true;
}

bool Engine::fetch_ready(int calls_back) {
  PTTS_REQUIRE(calls_back == 0 || calls_back == 1, "calls_back must be 0 or 1");
  const int q = calls_back ? prev_hb_ : out_hb_;
  hipError_t r;
  if (pipeline_) {
    r = hipEventQuery(ev_back_[q - q % nfr_]);
  } else {
    r = hipStreamQuery(stream_);
  }
  if (r == hipErrorNotReady) {
    (void)hipGetLastError();
    return false;
  }
  PTTS_HIP(r);
  return true;
}

// GEMM-core test hook: one dense GEMM (mode 0) on the given tile, split-K slabs (splits > 1:
// Y receives the [splits][M][N] partial slabs) or the split tail (tail_S > 0, the tiles with
// TileInfo::split_tail), from host operands; the tests compare it with an fp64 product (every
// shipped tile, shapes the model never runs). A request the tile cannot serve is refused.
void Engine::test_gemm(int layout, int M, int N, int K, int splits, int tail_S, const float* X, const float* Wt,
                       float* Y) {
  xh_dirty_ = true;
  PTTS_REQUIRE(ready_, "engine weights not finalized");
  PTTS_REQUIRE(X && Wt && Y && M >= 1 && N >= 1 && K >= 32 && K % 32 == 0, "test_gemm: bad shape");
  PTTS_REQUIRE(splits >= 1 && splits <= 16 && (splits == 1 || tail_S == 0), "test_gemm: bad split");
  const TileInfo& tile = tile_of(layout);
  PTTS_REQUIRE(tail_S <= 0 || tile.split_tail(), "test_gemm: tile " + std::to_string(layout) + " has no split tail");
  PTTS_REQUIRE(K % tile.bk == 0, "test_gemm: k must be a multiple of the tile's BK (" + std::to_string(tile.bk) + ")");
  sync();
  const int Nw = (N + 31) / 32 * 32;
  float *dx = nullptr, *dw = nullptr, *dy = nullptr;
  unsigned* dhm = nullptr;  // bf16x6 tiles: the split copy of W (split3)
  unsigned short* dlo = nullptr;
  PTTS_HIP(hipMalloc(&dx, sizeof(float) * M * K));
  PTTS_HIP(hipMalloc(&dw, sizeof(float) * Nw * K));
  PTTS_HIP(hipMalloc(&dy, sizeof(float) * splits * M * N));
  if (tile.split_weights()) {
    PTTS_HIP(hipMalloc(&dhm, sizeof(unsigned) * Nw * K));
    PTTS_HIP(hipMalloc(&dlo, sizeof(unsigned short) * Nw * K));
  }
  auto release = [&]() {
    (void)hipFree(dx), (void)hipFree(dw), (void)hipFree(dy);
    if (dhm) (void)hipFree(dhm);
    if (dlo) (void)hipFree(dlo);
  };
  try {
    PTTS_HIP(hipMemsetAsync(dw, 0, sizeof(float) * Nw * K, stream_));
    PTTS_HIP(hipMemcpyAsync(dx, X, sizeof(float) * M * K, hipMemcpyHostToDevice, stream_));
    PTTS_HIP(hipMemcpyAsync(dw, Wt, sizeof(float) * N * K, hipMemcpyHostToDevice, stream_));
    if (dhm) split3(dw, (long)Nw * K, dhm, dlo, stream_);
    GemmArgs a = dense_gemm(layout, M, N, K, dx, K, dw);
    a.Whm = dhm;
    a.Wlo = dlo;
    a.S = splits;
    if (splits > 1) {
      a.partial = dy;
    } else {
      a.Y = dy;
      a.ldy = N;
    }
    if (tail_S > 0) {
      a.tail_S = tail_S;
      a.tail_slab = fbm_.tslab;
      a.tail_cap = fbm_.tail_cap;
      a.tickets = fbm_.tickets;
      a.tickets_cap = TICKETS;
    }
    gemm(a, splits, stream_);
    PTTS_HIP(hipGetLastError());
    PTTS_HIP(hipMemcpyAsync(Y, dy, sizeof(float) * splits * M * N, hipMemcpyDeviceToHost, stream_));
    PTTS_HIP(hipStreamSynchronize(stream_));
  } catch (...) {
    (void)hipStreamSynchronize(stream_);
    release();
    throw;
  }
  release();
}

// Attention-path test hook: the product launchers, unchanged, on host operands (the tests compare
// with an fp64 softmax attention on operands the model never produces). kind 0: qkv_rope_append
// (dense rows, S == 0, or S partial slabs) + attention; kind 1: attention16_qkv (the fused
// Mimi step); kind 2: rope_table + attention_step_qkv. The KV store [n_slots][2][nh][cap][64] goes
// in and comes back; pre (optional) holds each slot's shared prefix [2][nh][F][64], F =
// pre_len[slot], back to back. Rows map to (slot, position) by the uniform RowMap {slot0, rps, p0,
// pos} or, kind 0, by the table `tab` (-1: padding), with the compact form when `ptab` [mpad] is
// given: tab holds the tokens only, ptab the padded 16-row groups, qrow / orow derived as the batched
// admission derives them. Every index the kernels form is checked here first.
void Engine::test_attention(int kind, int M, int nh, int cap, int window, int n_slots, int S, const float* qkv,
                            float* kvh, const float* pre, const int* pre_len, int slot0, int rps, int p0,
                            const int* pos, const int* tab, const int* ptab, int mpad, float* Qh, float* Oh) {
  PTTS_REQUIRE(ready_, "engine weights not finalized");
  PTTS_REQUIRE(kind >= 0 && kind <= 2 && qkv && kvh && Oh && (kind != 0 || Qh), "test_attention: bad arguments");
  PTTS_REQUIRE(M >= 1 && M <= 4096 && nh >= 1 && nh <= 16 && cap >= 1 && cap <= 65536 && window >= 0 &&
                   n_slots >= 1 && n_slots <= 64 && S >= 0 && S <= 16,
               "test_attention: bad shape");
  PTTS_REQUIRE(kind == 0 || (!tab && !ptab), "test_attention: the table form belongs to kind 0");
  PTTS_REQUIRE(kind != 1 || S == 0, "test_attention: the fused Mimi step takes dense rows");
  PTTS_REQUIRE(kind != 2 || (S >= 1 && window == 0 && rps == 1), "test_attention: the step takes slabs, one row per slot");
  PTTS_REQUIRE(!pre || (pre_len && kind != 1 && window == 0), "test_attention: a prefix needs the causal FlowLM kinds");
  PTTS_REQUIRE(!ptab || tab, "test_attention: ptab needs the token table");
  const bool pow2 = (cap & (cap - 1)) == 0;
  const bool ring = pow2 && window > 0 && !pre && kind != 2;  // positions may wrap
  auto group_ok = [](const int* t, int n0, int n1, int cap_, int slots_) {  // one 16-row group of a table
    int nv = 0;
    while (n0 + nv < n1 && t[n0 + nv] >= 0) ++nv;
    for (int i = n0 + nv; i < n1; ++i)
      if (t[i] != -1) return false;  // a slot's rows come first, padding after them
    for (int i = 0; i < nv; ++i) {
      const int v = t[n0 + i], sl = v >> 16, ps = v & 0xFFFF;
      if (sl >= slots_ || ps >= cap_ || v != t[n0] + i) return false;  // one slot, consecutive positions
    }
    return true;
  };
  int Mq = M;  // rows of Q and of the attention launch
  std::vector<int> qrow, orow;
  if (tab) {
    if (ptab) {
      PTTS_REQUIRE(mpad >= M && mpad <= 4096 && mpad % 16 == 0, "test_attention: bad padded row count");
      orow.assign(mpad, -1);
      int tc = 0;
      for (int r = 0; r < mpad; ++r) {
        if (ptab[r] < 0) continue;
        PTTS_REQUIRE(tc < M && tab[tc] == ptab[r], "test_attention: ptab's rows are not the tokens of tab");
        orow[r] = tc;
        qrow.push_back(r);
        ++tc;
      }
      PTTS_REQUIRE(tc == M, "test_attention: ptab's rows are not the tokens of tab");
      Mq = mpad;
    }
    const int* t = ptab ? ptab : tab;
    for (int r0 = 0; r0 < Mq; r0 += 16)
      PTTS_REQUIRE(group_ok(t, r0, std::min(r0 + 16, Mq), cap, n_slots), "test_attention: bad row table");
  } else {
    PTTS_REQUIRE(rps >= 1 && slot0 >= 0 && p0 >= 0 && slot0 + (M - 1) / rps < n_slots, "test_attention: bad row map");
    PTTS_REQUIRE(kind == 2 || rps % 16 == 0 || rps >= M, "test_attention: a 16-row group would straddle slots");
    for (int sl = slot0; sl <= slot0 + (M - 1) / rps; ++sl) {
      const int base = pos ? pos[sl] : p0, n = std::min(rps, M - (sl - slot0) * rps);
      PTTS_REQUIRE(base >= 0 && base < (1 << 30), "test_attention: bad position");
      if (kind == 2) {
        PTTS_REQUIRE(base <= cap, "test_attention: step position past the cache");
      } else if (ring) {  // (kind 1: attention16_qkv's own check, cap >= window + 16, is left to throw)
        PTTS_REQUIRE(kind == 1 || window + n - 1 <= cap, "test_attention: the pass would evict keys inside the window");
      } else {
        PTTS_REQUIRE(base + n <= cap, "test_attention: positions past the cache");
      }
    }
  }
  size_t pre_floats = 0;
  std::vector<size_t> pre_off(n_slots, 0);
  if (pre)
    for (int sl = 0; sl < n_slots; ++sl) {
      PTTS_REQUIRE(pre_len[sl] >= 0 && pre_len[sl] <= cap, "test_attention: bad prefix length");
      pre_off[sl] = pre_floats;
      pre_floats += (size_t)2 * nh * pre_len[sl] * 64;
    }
  sync();
  const int d = nh * 64;
  const size_t n_qkv = (size_t)std::max(S, 1) * M * 3 * d, n_kv = (size_t)n_slots * 2 * nh * cap * 64;
  std::vector<void*> allocs;
  std::vector<const float*> prep(n_slots, nullptr);
  auto dalloc = [&](size_t bytes) {
    void* p = nullptr;
    PTTS_HIP(hipMalloc(&p, std::max<size_t>(bytes, 16)));
    allocs.push_back(p);
    return p;
  };
  auto release = [&]() {
    for (void* p : allocs) (void)hipFree(p);
  };
  try {
    auto up = [&](const void* src, size_t bytes) {
      void* p = dalloc(bytes);
      PTTS_HIP(hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, stream_));
      return p;
    };
    const float* dqkv = (const float*)up(qkv, sizeof(float) * n_qkv);
    float* dkv = (float*)up(kvh, sizeof(float) * n_kv);
    float* dq = (float*)dalloc(sizeof(float) * Mq * d);
    float* dout = (float*)dalloc(sizeof(float) * M * d);
    PTTS_HIP(hipMemsetAsync(dq, 0, sizeof(float) * Mq * d, stream_));
    PTTS_HIP(hipMemsetAsync(dout, 0, sizeof(float) * M * d, stream_));
    RowMap map{slot0, rps, p0, nullptr};
    if (tab) {
      map = RowMap{0, 1, 0, nullptr, (const int*)up(tab, sizeof(int) * M)};
      if (ptab) {
        map.ptab = (const int*)up(ptab, sizeof(int) * mpad);
        map.mpad = mpad;
        map.qrow = (const int*)up(qrow.data(), sizeof(int) * M);
        map.orow = (const int*)up(orow.data(), sizeof(int) * mpad);
      }
    } else if (pos) {
      map.pos_arr = (const int*)up(pos, sizeof(int) * n_slots);
    }
    KvStore kv{dkv, (long)2 * nh * cap * 64, cap};
    if (pre) {
      const float* dpre = (const float*)up(pre, sizeof(float) * pre_floats);
      for (int sl = 0; sl < n_slots; ++sl) prep[sl] = dpre + pre_off[sl];
      kv.pre = (const float* const*)up(prep.data(), sizeof(float*) * n_slots);
      kv.pre_len = (const int*)up(pre_len, sizeof(int) * n_slots);
      kv.layer = 0;
    }
    if (kind == 0) {
      qkv_rope_append(S > 0 ? dqkv : nullptr, S, S > 0 ? nullptr : dqkv, M, nh, map, kv, dq, stream_);
      RowMap am = map;  // as flow_layers: the attention runs on the padded 16-row groups
      if (map.ptab) am.tab = map.ptab;
      attention(dq, Mq, nh, am, kv, window, dout, stream_);
    } else if (kind == 1) {
      attention16_qkv(dqkv, M, nh, map, kv, window, dout, stream_);
    } else {
      float* drope = (float*)dalloc(sizeof(float) * cap * 64);
      rope_table(drope, cap, stream_);
      attention_step_qkv(dqkv, S, M, nh, map, kv, drope, dout, stream_);
    }
    PTTS_HIP(hipGetLastError());
    PTTS_HIP(hipMemcpyAsync(kvh, dkv, sizeof(float) * n_kv, hipMemcpyDeviceToHost, stream_));
    if (kind == 0) PTTS_HIP(hipMemcpyAsync(Qh, dq, sizeof(float) * Mq * d, hipMemcpyDeviceToHost, stream_));
    PTTS_HIP(hipMemcpyAsync(Oh, dout, sizeof(float) * M * d, hipMemcpyDeviceToHost, stream_));
    PTTS_HIP(hipStreamSynchronize(stream_));
  } catch (...) {
    (void)hipStreamSynchronize(stream_);
    release();
    throw;
  }
  release();
}

// Row-reduce test hook: the product launcher row_reduce (k_row_reduce, or k_row_reduce4 for a
// 512-wide row outside the front part) on host operands; absent operands are null. The tests
// compare with the fp64 formula on shapes and operand sets the model never runs.
void Engine::test_row_reduce(int M, int N, int S, int act, int ln, float eps, int front, const float* P,
                             const float* bias, const float* gate, const float* R, const float* ln_w,
                             const float* ln_b, const float* mscale, const float* mshift, float* Y, float* H,
                             float* Hfrag) {
  PTTS_REQUIRE(ready_, "engine weights not finalized");
  PTTS_REQUIRE(P && Y && M >= 1 && M <= 4096 && N >= 4 && N <= 8192 && N % 4 == 0 && S >= 1 && S <= 16,
               "test_row_reduce: bad shape");
  PTTS_REQUIRE(act == ACT_NONE || act == ACT_GELU, "test_row_reduce: act is none or GELU");
  PTTS_REQUIRE(!ln || (N <= 1024 && H), "test_row_reduce: LayerNorm rows are at most 1024 wide");
  PTTS_REQUIRE((ln_w == nullptr) == (ln_b == nullptr) && (mscale == nullptr) == (mshift == nullptr),
               "test_row_reduce: ln_w with ln_b, mscale with mshift");
  PTTS_REQUIRE(ln || (!ln_w && !mshift && !Hfrag), "test_row_reduce: affine, modulate and hfrag need ln");
  PTTS_REQUIRE(!Hfrag || (N == FK_K && M <= 32), "test_row_reduce: hfrag needs n == 1024 and m <= 32");
  sync();
  std::vector<void*> allocs;
  auto release = [&]() {
    for (void* p : allocs) (void)hipFree(p);
  };
  try {
    auto dalloc = [&](size_t floats) {
      void* p = nullptr;
      PTTS_HIP(hipMalloc(&p, sizeof(float) * std::max<size_t>(floats, 4)));
      allocs.push_back(p);
      return (float*)p;
    };
    auto up = [&](const float* src, size_t floats) -> float* {
      if (!src) return nullptr;
      float* p = dalloc(floats);
      PTTS_HIP(hipMemcpyAsync(p, src, sizeof(float) * floats, hipMemcpyHostToDevice, stream_));
      return p;
    };
    const size_t mn = (size_t)M * N;
    RowReduceArgs a{};
    a.P = up(P, (size_t)S * mn);
    a.S = S, a.M = M, a.N = N;
    a.bias = up(bias, N);
    a.act = act;
    a.gate = up(gate, mn), a.ldg = N;
    a.R = up(R, mn), a.ldr = N;
    a.Y = dalloc(mn), a.ldy = N;
    a.ln = ln ? 1 : 0;
    a.ln_w = up(ln_w, N), a.ln_b = up(ln_b, N);
    a.eps = eps;
    a.mscale = up(mscale, mn), a.mshift = up(mshift, mn), a.ldm = N;
    a.front = front ? 1 : 0;
    if (ln) a.Hout = dalloc(mn), a.ldh = N;
    if (Hfrag) {
      a.Hfrag = dalloc(FK_A_FLOATS);
      PTTS_HIP(hipMemsetAsync(a.Hfrag, 0, sizeof(float) * FK_A_FLOATS, stream_));
    }
    row_reduce(a, stream_);
    PTTS_HIP(hipGetLastError());
    PTTS_HIP(hipMemcpyAsync(Y, a.Y, sizeof(float) * mn, hipMemcpyDeviceToHost, stream_));
    if (ln) PTTS_HIP(hipMemcpyAsync(H, a.Hout, sizeof(float) * mn, hipMemcpyDeviceToHost, stream_));
    if (Hfrag) PTTS_HIP(hipMemcpyAsync(Hfrag, a.Hfrag, sizeof(float) * FK_A_FLOATS, hipMemcpyDeviceToHost, stream_));
    PTTS_HIP(hipStreamSynchronize(stream_));
  } catch (...) {
    (void)hipStreamSynchronize(stream_);
    release();
    throw;
  }
  release();
}

double Engine::time_op(int B, const std::string& name, int reps) {
  xh_dirty_ = true;  // replays write fbm_.x / fbm_.h
  PTTS_REQUIRE(ready_, "engine weights not finalized");
  PTTS_REQUIRE(B >= 1 && B <= max_slots_, "n_rows out of range");
  PTTS_REQUIRE(reps >= 1, "reps must be >= 1");
  PTTS_HIP(hipSetDevice(dev_));
  std::vector<Op> ops = build_step(B);
  const Op* sel = nullptr;
  bool back = false, in_back = false;
  for (const Op& op : ops) {
    in_back = in_back || op.name == "mimi.quant_upsample";
    if (op.name == name) sel = &op, back = in_back;
  }
  PTTS_REQUIRE(sel != nullptr, "no op named " + name + " in the step plan");
  // PTTS_TIME_CAP: time back-part ops with the per-CU cap of pipelined stepping
  const bool capped = back && pipeline_ && probe_env("PTTS_TIME_CAP");
  set_wg_cap(capped ? back_cap_ : 0);
  hipEvent_t e0, e1;
  PTTS_HIP(hipEventCreate(&e0));
  PTTS_HIP(hipEventCreate(&e1));
  float ms = 0.f;
  if (sel->prep) {  // each replay behind its own prep: (prep, op) x reps minus prep x reps
    sel->prep(stream_);
    sel->fn(stream_);  // warm
    PTTS_HIP(hipEventRecord(e0, stream_));
    for (int i = 0; i < reps; ++i) {
      sel->prep(stream_);
      sel->fn(stream_);
    }
    PTTS_HIP(hipEventRecord(e1, stream_));
    PTTS_HIP(hipEventSynchronize(e1));
    float both = 0.f, prep = 0.f;
    PTTS_HIP(hipEventElapsedTime(&both, e0, e1));
    PTTS_HIP(hipEventRecord(e0, stream_));
    for (int i = 0; i < reps; ++i) sel->prep(stream_);
    PTTS_HIP(hipEventRecord(e1, stream_));
    PTTS_HIP(hipEventSynchronize(e1));
    PTTS_HIP(hipEventElapsedTime(&prep, e0, e1));
    ms = both - prep;
    sel->prep(stream_);  // leave the op's state as a step finds it (flow.layers: its set empty)
    PTTS_HIP(hipStreamSynchronize(stream_));
  } else {
    sel->fn(stream_);  // warm
    PTTS_HIP(hipEventRecord(e0, stream_));
    for (int i = 0; i < reps; ++i) sel->fn(stream_);
    PTTS_HIP(hipEventRecord(e1, stream_));
    PTTS_HIP(hipEventSynchronize(e1));
    PTTS_HIP(hipEventElapsedTime(&ms, e0, e1));
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  set_wg_cap(0);
  return 1000.0 * ms / reps;
}

// Measurement hook: the step plan split at the FlowLM/flow-head -> Mimi boundary into two graphs;
// times each alone and both launched together on two streams (no dependency, data races are
// irrelevant for timing). us[0] = front alone, us[1] = back alone, us[2] = both concurrently.
void Engine::overlap_probe(int B, int reps, double* us) {
  xh_dirty_ = true;  // replays write fbm_.x / fbm_.h
  PTTS_REQUIRE(ready_, "engine weights not finalized");
  PTTS_REQUIRE(B >= 1 && B <= max_slots_ && reps >= 1, "bad probe arguments");
  PTTS_HIP(hipSetDevice(dev_));
  std::vector<Op> ops = build_step(B);
  size_t cut = 0;
  while (cut < ops.size() && ops[cut].name != "mimi.quant_upsample") ++cut;
  PTTS_REQUIRE(cut < ops.size(), "step plan has no Mimi stage");
  hipStream_t s2 = nullptr, s_hi = nullptr, s_lo = nullptr;
  PTTS_HIP(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
  int prio_lo = 0, prio_hi = 0;
  PTTS_HIP(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
  PTTS_HIP(hipStreamCreateWithPriority(&s_hi, hipStreamNonBlocking, prio_hi));
  PTTS_HIP(hipStreamCreateWithPriority(&s_lo, hipStreamNonBlocking, prio_lo));
  hipGraphExec_t ge[2] = {};
  hipGraph_t g[2] = {};
  for (int part = 0; part < 2; ++part) {  // as captured for pipelined stepping (back part capped)
    PTTS_HIP(hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal));
    set_wg_cap(part == 1 ? back_cap_ : 0);
    for (size_t i = part ? cut : 0; i < (part ? ops.size() : cut); ++i) {
      // each replay of the persistent FlowLM launch needs its hand-off set empty
      if (ops[i].name == "flow.layers") ops[i].prep(stream_);
      ops[i].fn(stream_);
    }
    set_wg_cap(0);
    PTTS_HIP(hipStreamEndCapture(stream_, &g[part]));
    PTTS_HIP(hipGraphInstantiate(&ge[part], g[part], nullptr, nullptr, 0));
  }
  hipEvent_t e0, e1, e2;
  PTTS_HIP(hipEventCreate(&e0));
  PTTS_HIP(hipEventCreate(&e1));
  PTTS_HIP(hipEventCreate(&e2));
  auto timed = [&](int mode) {
    hipStream_t sa = mode == 3 ? s_hi : stream_, sb = mode == 3 ? s_lo : s2;
    for (int w = 0; w < 2; ++w) {
      if (mode != 1) PTTS_HIP(hipGraphLaunch(ge[0], sa));
      if (mode != 0) PTTS_HIP(hipGraphLaunch(ge[1], sb));
    }
    PTTS_HIP(hipStreamSynchronize(sa));
    PTTS_HIP(hipStreamSynchronize(sb));
    PTTS_HIP(hipEventRecord(e0, sa));
    PTTS_HIP(hipStreamWaitEvent(sb, e0, 0));
    for (int r = 0; r < reps; ++r) {
      if (mode != 1) PTTS_HIP(hipGraphLaunch(ge[0], sa));
      if (mode != 0) PTTS_HIP(hipGraphLaunch(ge[1], sb));
    }
    PTTS_HIP(hipEventRecord(e2, sb));
    PTTS_HIP(hipStreamWaitEvent(sa, e2, 0));
    PTTS_HIP(hipEventRecord(e1, sa));
    PTTS_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    PTTS_HIP(hipEventElapsedTime(&ms, e0, e1));
    return 1000.0 * ms / reps;
  };
  // us[7]: front || Mimi transformer || SEANet decoder on three streams (a 3-stage pipeline)
  if (probe_env("PTTS_PROBE_MODES") && strchr(probe_env("PTTS_PROBE_MODES"), '7')) {
    size_t cut2 = cut;
    while (cut2 < ops.size() && ops[cut2].name != "seanet.conv0") ++cut2;
    hipGraphExec_t g3[2] = {};
    hipGraph_t d3[2] = {};
    for (int part = 0; part < 2; ++part) {
      PTTS_HIP(hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal));
      set_wg_cap(back_cap_);
      for (size_t i = part ? cut2 : cut; i < (part ? ops.size() : cut2); ++i) ops[i].fn(stream_);
      set_wg_cap(0);
      PTTS_HIP(hipStreamEndCapture(stream_, &d3[part]));
      PTTS_HIP(hipGraphInstantiate(&g3[part], d3[part], nullptr, nullptr, 0));
    }
    hipStream_t s3 = nullptr;
    PTTS_HIP(hipStreamCreateWithFlags(&s3, hipStreamNonBlocking));
    hipEvent_t a0, a1, a2, a3;
    PTTS_HIP(hipEventCreate(&a0));
    PTTS_HIP(hipEventCreate(&a1));
    PTTS_HIP(hipEventCreate(&a2));
    PTTS_HIP(hipEventCreate(&a3));
    auto run3 = [&](int n) {
      for (int r = 0; r < n; ++r) {
        PTTS_HIP(hipGraphLaunch(ge[0], stream_));
        PTTS_HIP(hipGraphLaunch(g3[0], s2));
        PTTS_HIP(hipGraphLaunch(g3[1], s3));
      }
    };
    run3(2);
    PTTS_HIP(hipDeviceSynchronize());
    PTTS_HIP(hipEventRecord(a0, stream_));
    PTTS_HIP(hipStreamWaitEvent(s2, a0, 0));
    PTTS_HIP(hipStreamWaitEvent(s3, a0, 0));
    run3(reps);
    PTTS_HIP(hipEventRecord(a2, s2));
    PTTS_HIP(hipEventRecord(a3, s3));
    PTTS_HIP(hipStreamWaitEvent(stream_, a2, 0));
    PTTS_HIP(hipStreamWaitEvent(stream_, a3, 0));
    PTTS_HIP(hipEventRecord(a1, stream_));
    PTTS_HIP(hipEventSynchronize(a1));
    float ms = 0.f;
    PTTS_HIP(hipEventElapsedTime(&ms, a0, a1));
    us[7] = 1000.0 * ms / reps;
    for (hipEvent_t e : {a0, a1, a2, a3}) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(s3);
    for (int part = 0; part < 2; ++part) {
      (void)hipGraphExecDestroy(g3[part]);
      (void)hipGraphDestroy(d3[part]);
    }
  }
  // PTTS_PROBE_MODES: digits of the measurements to run (default all: "0123456")
  const std::string modes = probe_env("PTTS_PROBE_MODES") ? probe_env("PTTS_PROBE_MODES") : "0123456";
  auto want = [&](int m) { return modes.find((char)('0' + m)) != std::string::npos; };
  for (int m = 0; m < 7; ++m) us[m] = -1.0;  // us[7]: see above
  for (int m = 0; m < 4; ++m)
    if (want(m)) us[m] = timed(m);
  // us[4..6]: front graph || back part launched op by op on a stream whose CU mask keeps
  // 8/8, 6/8, 4/8 of the CUs (graph launches do not honour a stream's CU mask)
  for (int v = 0; v < 3; ++v) {
    if (!want(4 + v)) continue;
    const int keep = 8 - 2 * v;
    std::vector<uint32_t> mask(8, 0u);  // 256 CUs
    for (int cu = 0; cu < 256; ++cu)
      if ((cu % 8) < keep) mask[cu / 32] |= 1u << (cu % 32);
    hipStream_t sm = nullptr;
    PTTS_HIP(hipExtStreamCreateWithCUMask(&sm, (uint32_t)mask.size(), mask.data()));
    auto back_eager = [&]() {  // capped as in pipelined stepping: the persistent flow-head launch of
      set_wg_cap(back_cap_);    // the concurrent front graph needs room for all its workgroups
      for (size_t i = cut; i < ops.size(); ++i) ops[i].fn(sm);
      set_wg_cap(0);
    };
    for (int w = 0; w < 2; ++w) {
      PTTS_HIP(hipGraphLaunch(ge[0], stream_));
      back_eager();
    }
    PTTS_HIP(hipStreamSynchronize(stream_));
    PTTS_HIP(hipStreamSynchronize(sm));
    PTTS_HIP(hipEventRecord(e0, stream_));
    PTTS_HIP(hipStreamWaitEvent(sm, e0, 0));
    for (int r = 0; r < reps; ++r) {
      PTTS_HIP(hipGraphLaunch(ge[0], stream_));
      back_eager();
    }
    PTTS_HIP(hipEventRecord(e2, sm));
    PTTS_HIP(hipStreamWaitEvent(stream_, e2, 0));
    PTTS_HIP(hipEventRecord(e1, stream_));
    PTTS_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    PTTS_HIP(hipEventElapsedTime(&ms, e0, e1));
    us[4 + v] = 1000.0 * ms / reps;
    (void)hipStreamDestroy(sm);
  }
  // PTTS_PROBE_SPLITS="F:K,...": spatial partition. The front part launched op by op on a stream
  // whose CU mask keeps the CUs with cu % 8 < F, the back part op by op on the CUs with
  // cu % 8 >= 8 - K (disjoint when F + K <= 8); F or K = 0 leaves that part out (alone timings).
  // One line per split on stderr: microseconds per step (front + back per call).
  if (probe_env("PTTS_PROBE_SPLITS")) {
    auto make_masked = [&](int lo, int hi) {  // CUs with lo <= cu % 8 < hi
      std::vector<uint32_t> m(8, 0u);
      for (int cu = 0; cu < 256; ++cu)
        if ((cu % 8) >= lo && (cu % 8) < hi) m[cu / 32] |= 1u << (cu % 32);
      hipStream_t st = nullptr;
      PTTS_HIP(hipExtStreamCreateWithCUMask(&st, (uint32_t)m.size(), m.data()));
      return st;
    };
    const std::string spec = probe_env("PTTS_PROBE_SPLITS");
    size_t p = 0;
    while (p < spec.size()) {
      size_t q = spec.find(',', p);
      if (q == std::string::npos) q = spec.size();
      const std::string item = spec.substr(p, q - p);
      p = q + 1;
      // the back side may be a stand-in on the other CUs: "F:eN" N empty launches per step, "F:mN"
      // one copy kernel moving N MB (read + write) per step
      const std::string bs = item.substr(item.find(':') + 1);
      const char kind = bs.empty() ? '0' : bs[0];
      const bool dummy = kind == 'e' || kind == 'm';
      const int F = atoi(item.c_str()), K = dummy ? 8 - F : atoi(bs.c_str()), N = dummy ? atoi(bs.c_str() + 1) : 0;
      float* big = nullptr;
      if (kind == 'm') PTTS_HIP(hipMalloc(&big, (size_t)N << 20));
      fprintf(stderr, "split %d:%s: streams\n", F, bs.c_str());
      hipStream_t sf = F > 0 ? make_masked(0, F) : nullptr, sb = K > 0 ? make_masked(8 - K, 8) : nullptr;
      fprintf(stderr, "split %d:%s: warm\n", F, bs.c_str());
      auto one = [&]() {
        if (sf)
          for (size_t i = 0; i < cut; ++i) ops[i].fn(sf);
        if (sb && kind == 'e') {
          for (int i = 0; i < N; ++i) copy2d(fbm_.x, 1, fbm_.q, 1, 1, 1, sb);
        } else if (sb && kind == 'm') {
          const long half = ((long)N << 20) / 8;  // floats copied: N/2 MB read + N/2 MB written
          copy2d(big, 1024, big + half, 1024, (int)(half / 1024), 1024, sb);
        } else if (sb) {
          set_wg_cap(back_cap_);
          for (size_t i = cut; i < ops.size(); ++i) ops[i].fn(sb);
          set_wg_cap(0);
        }
      };
      for (int w = 0; w < 2; ++w) one();
      PTTS_HIP(hipDeviceSynchronize());
      hipStream_t s0 = sf ? sf : sb, s1 = sb ? sb : sf;
      PTTS_HIP(hipEventRecord(e0, s0));
      PTTS_HIP(hipStreamWaitEvent(s1, e0, 0));
      for (int r = 0; r < reps; ++r) one();
      PTTS_HIP(hipEventRecord(e2, s1));
      PTTS_HIP(hipStreamWaitEvent(s0, e2, 0));
      PTTS_HIP(hipEventRecord(e1, s0));
      PTTS_HIP(hipEventSynchronize(e1));
      float ms = 0.f;
      PTTS_HIP(hipEventElapsedTime(&ms, e0, e1));
      fprintf(stderr, "split front %d/8 back %d/8 (%s): %.1f us per step\n", F, K, dummy ? bs.c_str() : "ops",
              1000.0 * ms / reps);
      if (sf) (void)hipStreamDestroy(sf);
      if (sb) (void)hipStreamDestroy(sb);
      if (big) (void)hipFree(big);
    }
  }
  for (int part = 0; part < 2; ++part) {
    (void)hipGraphExecDestroy(ge[part]);
    (void)hipGraphDestroy(g[part]);
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipEventDestroy(e2);
  (void)hipStreamDestroy(s2);
  (void)hipStreamDestroy(s_hi);
  (void)hipStreamDestroy(s_lo);
}

// ------------------------------------------------------------------ voices and slots
void Engine::encoder_transformer(std::vector<Op>& ops, float* x, int T, float* h, float* qkv, float* q, float* o,
                                 float* u, float* ring) {
  RowMap map{0, T, 0, nullptr};
  {
    const float *w = W(L_.menc[0].n1w), *b = W(L_.menc[0].n1b);
    ops.push_back({"enc.ln1", [=](hipStream_t s) { layernorm(x, MD, h, MD, T, MD, w, b, 1e-5f, s); }});
  }
  for (int l = 0; l < MNL; ++l) {
    const Layout::TL& t = L_.menc[l];
    KvStore kv{ring + (size_t)l * 2 * MNH * T * 64, 0, T};
    dense_op(ops, "enc.qkv", h, T, W(t.in_proj), 3 * MD, MD, nullptr, ACT_NONE, nullptr, nullptr, qkv);
    ops.push_back({"enc.rope", [=](hipStream_t s) { qkv_rope_append(nullptr, 0, qkv, T, MNH, map, kv, q, s); }});
    ops.push_back({"enc.attn", [=](hipStream_t s) { attention(q, T, MNH, map, kv, MCTX, o, s); }});
    dense_op(ops, "enc.out", o, T, W(t.out_proj), MD, MD, nullptr, ACT_NONE, W(t.ls1), x, x);
    {
      const float *w = W(t.n2w), *b = W(t.n2b);
      ops.push_back({"enc.ln2", [=](hipStream_t s) { layernorm(x, MD, h, MD, T, MD, w, b, 1e-5f, s); }});
    }
    dense_op(ops, "enc.ff1", h, T, W(t.l1), MFF, MD, nullptr, ACT_GELU, nullptr, nullptr, u);
    dense_op(ops, "enc.ff2", u, T, W(t.l2), MD, MFF, nullptr, ACT_NONE, W(t.ls2), x, x);
    if (l + 1 < MNL) {
      const float *w = W(L_.menc[l + 1].n1w), *b = W(L_.menc[l + 1].n1b);
      ops.push_back({"enc.ln1", [=](hipStream_t s) { layernorm(x, MD, h, MD, T, MD, w, b, 1e-5f, s); }});
    }
  }
}

namespace {
// adaptive_voice_prompt_chunk_frames (tts_model.rs:562-577); override > 0 wins, < 0 = one pass.
int voice_chunk_frames(int F, int override_frames) {
  if (override_frames > 0) return override_frames;
  if (override_frames < 0 || F <= 120) return std::max(F, 1);
  if (F <= 600) return 120;
  if (F <= 1800) return 180;
  return 240;
}
size_t al16(size_t bytes) { return (bytes + 15) / 16 * 16; }
}  // namespace

// What the host works out about a clip before a clone is enqueued
struct VoicePlan {
  int n_in = 0, s16 = 0;
  ResamplePlan rp{};
  bool septic = false;       // the rubato rule (identity rates take neither resampler)
  std::vector<float> taps;   // polyphase rule
  std::vector<int> sst;      // rubato position schedule
  std::vector<float> sfr;
  int n = 0, Np = 0, F = 0, Te = 0, cf = 0;  // 24 kHz samples, frame-padded samples, frames, encoder rows, chunk frames
  // the upload (VoiceWs::up): samples | taps | rubato start | rubato frac | on the device: o_fx
  size_t o_taps = 0, o_st = 0, o_fr = 0, o_fx = 0, up_bytes = 0, dev_bytes = 0;
};

namespace {
VoicePlan voice_plan(int n_in, int fmt, int sr, int chunk_frames, int resampler, int max_ctx) {
  PTTS_REQUIRE(n_in >= 1, "empty PCM");
  PTTS_REQUIRE(fmt == PTTS_SAMPLES_F32 || fmt == PTTS_SAMPLES_S16, "unknown sample format");
  PTTS_REQUIRE(sr > 0, "sample rate must be positive");
  PTTS_REQUIRE(resampler == PTTS_RESAMPLE_POLY || resampler == PTTS_RESAMPLE_RUBATO_SEPTIC, "unknown resampler");
  VoicePlan p;
  p.n_in = n_in;
  p.s16 = fmt == PTTS_SAMPLES_S16 ? 1 : 0;
  p.rp = resample_plan(sr, PTTS_SAMPLE_RATE);
  p.septic = resampler == PTTS_RESAMPLE_RUBATO_SEPTIC && !p.rp.identity();
  const long n_long = p.rp.identity() ? n_in : p.septic ? septic_schedule(n_in, sr, PTTS_SAMPLE_RATE, &p.sst, &p.sfr)
                                                        : p.rp.out_len(n_in);
  PTTS_REQUIRE(n_long >= 1 && n_long < (1L << 28) && p.rp.L <= (1 << 22), "voice prompt length or rate out of range");
  p.n = (int)n_long;
  p.Np = (p.n + FRAME - 1) / FRAME * FRAME;  // zero-pad to whole frames (mimi.py:103)
  p.F = p.Np / FRAME, p.Te = p.Np / 120;
  PTTS_REQUIRE(p.F < max_ctx, "voice prompt longer than max_ctx");
  p.cf = voice_chunk_frames(p.F, chunk_frames);
  if (!p.septic && !p.rp.identity()) p.taps = resample_taps(p.rp);
  p.o_taps = al16((size_t)n_in * (p.s16 ? 2 : 4));
  p.o_st = p.o_taps + al16(p.taps.size() * sizeof(float));
  p.o_fr = p.o_st + al16(p.sst.size() * sizeof(int));
  p.up_bytes = p.o_fr + al16(p.sfr.size() * sizeof(float));
  p.o_fx = p.up_bytes;
  p.dev_bytes = p.up_bytes + (p.septic ? al16((size_t)n_in * sizeof(float)) : 0);
  return p;
}
}  // namespace

// The GPU resampler on its own (test hook of the voice front end): the resample_poly rule, or the
// Rust driver's rubato FastFixedIn / Septic (kernels.h septic_schedule). Equal rates copy the input,
// as audio.rs:198-200 returns the tensor unchanged.
void Engine::resample_host(const float* x, int n, int sr_from, int sr_to, float* y, int resampler) {
  PTTS_REQUIRE(x && y && n >= 1, "empty input");
  PTTS_REQUIRE(sr_from > 0 && sr_to > 0, "sample rates must be positive");
  PTTS_REQUIRE(resampler == PTTS_RESAMPLE_POLY || resampler == PTTS_RESAMPLE_RUBATO_SEPTIC, "unknown resampler");
  const bool septic = resampler == PTTS_RESAMPLE_RUBATO_SEPTIC && sr_from != sr_to;
  const ResamplePlan rp = resample_plan(sr_from, sr_to);
  std::vector<int> st;
  std::vector<float> fr;
  const long n_out = septic ? septic_schedule(n, sr_from, sr_to, &st, &fr) : sr_from == sr_to ? n : rp.out_len(n);
  PTTS_REQUIRE(n_out >= 1, "input too short for the resampler (no output samples)");
  PTTS_REQUIRE(rp.L <= (1 << 22) && n_out < (1L << 30), "resampling ratio or length too large");
  sync();
  std::vector<float> taps;
  if (!septic && sr_from != sr_to) taps = resample_taps(rp);
  void *dx = nullptr, *dh = nullptr, *dy = nullptr, *ds = nullptr;
  try {
    PTTS_HIP(hipMalloc(&dx, sizeof(float) * n));
    PTTS_HIP(hipMalloc(&dy, sizeof(float) * n_out));
    PTTS_HIP(hipMemcpyAsync(dx, x, sizeof(float) * n, hipMemcpyHostToDevice, stream_));
    if (sr_from == sr_to) {
      PTTS_HIP(hipMemcpyAsync(dy, dx, sizeof(float) * n, hipMemcpyDeviceToDevice, stream_));
    } else if (septic) {
      PTTS_HIP(hipMalloc(&ds, sizeof(int) * n_out));
      PTTS_HIP(hipMalloc(&dh, sizeof(float) * n_out));
      PTTS_HIP(hipMemcpyAsync(ds, st.data(), sizeof(int) * n_out, hipMemcpyHostToDevice, stream_));
      PTTS_HIP(hipMemcpyAsync(dh, fr.data(), sizeof(float) * n_out, hipMemcpyHostToDevice, stream_));
      resample_septic((const float*)dx, n, (const int*)ds, (const float*)dh, (int)n_out, (int)n_out, (float*)dy,
                      stream_);
    } else {
      PTTS_HIP(hipMalloc(&dh, sizeof(float) * taps.size()));
      PTTS_HIP(hipMemcpyAsync(dh, taps.data(), sizeof(float) * taps.size(), hipMemcpyHostToDevice, stream_));
      resample((const float*)dx, n, (const float*)dh, rp, (int)n_out, (int)n_out, (float*)dy, stream_);
    }
    PTTS_HIP(hipGetLastError());
    PTTS_HIP(hipMemcpyAsync(y, dy, sizeof(float) * n_out, hipMemcpyDeviceToHost, stream_));
    PTTS_HIP(hipStreamSynchronize(stream_));
  } catch (...) {
    (void)hipStreamSynchronize(stream_);
    (void)hipFree(dx), (void)hipFree(dh), (void)hipFree(dy), (void)hipFree(ds);
    throw;
  }
  (void)hipFree(dx), (void)hipFree(dh), (void)hipFree(dy), (void)hipFree(ds);
}

// ------------------------------------------------------------------ voice cloning
// One clone, two ways of calling it: samples at `sr` -> resampled to 24 kHz
// on the GPU -> zero-padded to whole frames (tts_model.rs:515-527) -> Mimi encoder (mimi.rs:113-141)
// -> speaker projection (:543-553) -> FlowLM prompt prefill (:580-599) into the voice's compact
// cache. voice_clone enqueues it on the stream, in the VoiceWs, it is given. voice_from_* drain the
// pipeline, run it on stream_ in a transient workspace and wait; voice_job_* run it on stream_vc_
// in the grow-only vws_, staged through pinned memory, with no sync() and no allocation but the
// voice's own (slots_open orders the front stream behind the job's event).
namespace {
void free_voice(ptts_voice* v) {
  if (v->ev) {  // a pending job still writes the cache and the pinned conditioning
    (void)hipEventSynchronize(v->ev);
    (void)hipEventDestroy(v->ev);
  }
  if (v->h_cond) (void)hipHostFree(v->h_cond);
  if (v->kv) (void)hipFree(v->kv);
  delete v;
}
}  // namespace

void Engine::vws_free(VoiceWs& w) {
  if (w.block) (void)hipFree(w.block);
  if (w.up) (void)hipFree(w.up);
  for (char*& h : w.h_up)
    if (h) (void)hipHostFree(h), h = nullptr;
  w.block = nullptr, w.up = nullptr;
  w.frames = 0, w.up_bytes = 0, w.h_bytes = 0;
}

// Grow-only. A longer clip (or a larger upload) than any before re-allocates the workspace at the
// larger sizes, after the work already queued on `st` (the stream that uses the workspace) has
// run: the only point at which a voice job synchronizes its stream. host_bytes 0 (synchronous
// clones): no pinned staging blocks.
void Engine::vws_reserve(VoiceWs& w, hipStream_t st, int frames, size_t host_bytes, size_t up_bytes) {
  if (frames <= w.frames && host_bytes <= w.h_bytes && up_bytes <= w.up_bytes) return;
  PTTS_HIP(hipStreamSynchronize(st));
  frames = std::max(frames, w.frames), host_bytes = std::max(host_bytes, w.h_bytes);
  up_bytes = std::max(up_bytes, w.up_bytes);
  vws_free(w);
  if (host_bytes)  // the two pinned staging blocks
    for (char*& h : w.h_up) PTTS_HIP(hipHostMalloc((void**)&h, host_bytes, hipHostMallocDefault));
  w.h_bytes = host_bytes;
  // the device block: the upload, then the converted clip (rubato rule)
  if (up_bytes) PTTS_HIP(hipMalloc((void**)&w.up, up_bytes));
  w.up_bytes = up_bytes;
  // one allocation, carved in 256-byte steps: first pass sizes it, second pass hands out the pointers
  size_t off = 0;
  auto take = [&](size_t cnt) {
    float* p = w.block ? w.block + off : nullptr;
    off += (std::max<size_t>(cnt, 1) + 63) / 64 * 64;
    return p;
  };
  FlowBufs& b = w.fb;
  auto carve = [&] {
    const size_t Fc = (size_t)frames, Np = Fc * FRAME, Te = Fc * 16;
    w.pcm = take(Np);
    w.A = take(Np * 64);
    w.Bf = take(Np * 64);
    w.V = take(Np * 32);
    w.zeros = take(16 * 512);
    w.eh = take(Te * MD);
    w.eqkv = take(Te * 3 * MD);
    w.eq = take(Te * MD);
    w.eo = take(Te * MD);
    w.eu = take(Te * MFF);
    w.ering = take((size_t)MNL * 2 * MNH * Te * 64);
    w.Hd = take(Fc * 16 * 512);  // one replicated row block per chunk, chunks of >= 1 frame
    w.lat = take(Fc * 512);
    const size_t R = (Fc + 15) / 16 * 16, Rp = std::min<size_t>(R, PREFILL);
    b.x = take(R * D);  // the conditioning rows (the speaker projection's output), then the residual stream
    w.cond = b.x;
    b.h = take(Rp * D);
    b.q = take(Rp * D);
    b.o = take(Rp * D);
    b.u = take(Rp * FF);
    // the slabs of a pass of < 256 rows, or the one [rows][FF] block of a longer one (linear_split)
    b.pcap = std::max((size_t)4 << 20, Rp * FF);
    b.partial = take(b.pcap);
    // split-tail scratch of the passes of >= 256 rows: at most 64 N tiles per 128 rows, 4 slices
    b.tail_cap = Fc < 256 ? 0 : (long)std::min<size_t>(TAIL_CAP, (Fc + 127) / 128 * 64 * 4 * 128 * 64);
    b.tslab = take((size_t)b.tail_cap);
    b.tickets = (int*)take(TICKETS);
  };
  carve();
  PTTS_HIP(hipMalloc((void**)&w.block, off * sizeof(float)));
  off = 0;
  carve();
  PTTS_HIP(hipMemsetAsync(w.zeros, 0, sizeof(float) * 16 * 512, st));
  PTTS_HIP(hipMemsetAsync(b.tickets, 0, sizeof(int) * TICKETS, st));  // every launch leaves them zero
  w.frames = frames;
}

// The voice's own allocations (a job's: its event, and pinned memory for a PCM voice's conditioning)
ptts_voice* Engine::voice_new(int F, bool pcm, bool job) {
  ptts_voice* v = new ptts_voice();
  v->F = F;
  v->owner = this;
  try {
    PTTS_HIP(hipMalloc(&v->kv, sizeof(float) * (size_t)NL * 2 * NH * F * 64));
    if (pcm && job) PTTS_HIP(hipHostMalloc((void**)&v->h_cond, sizeof(float) * (size_t)F * D, hipHostMallocDefault));
    if (pcm && !job) v->cond.resize((size_t)F * D);
    if (job) PTTS_HIP(hipEventCreateWithFlags(&v->ev, hipEventDisableTiming));
  } catch (...) {
    free_voice(v);
    throw;
  }
  return v;
}

// The clone of the clip uploaded to w.up (plan p), or with p == nullptr only the prompt prefill of
// the v->F conditioning rows already in w.fb.x; everything on `st`. h_cond: where the conditioning
// rows are copied (nullptr: nowhere). Records v->ev behind it all when the voice has one.
// The reference encodes chunk by chunk (adaptive chunk length, tts_model.rs:530-541) with step=0
// for every chunk: the streaming convs and the encoder transformer carry their state, which equals
// the single pass below, but ConvDownsample1d re-applies its replicate padding at each chunk's
// first frame (conv.rs:116-123); the downsample conv is therefore run per chunk.
void Engine::voice_clone(const VoicePlan* p, const VoiceWs& w, hipStream_t st, ptts_voice* v, float* h_cond) {
  const int F = v->F;
  if (p) {
    const int n_in = p->n_in, n = p->n, Np = p->Np, Te = p->Te, cf = p->cf;
    float* dpcm = w.pcm;
    if (p->septic) {  // the rubato rule keeps its kernel, fed by a converting copy
      float* fx = (float*)(w.up + p->o_fx);  // behind the upload, in the same device block
      voice_ingest(w.up, p->s16, n_in, nullptr, ResamplePlan{}, n_in, n_in, fx, st);
      resample_septic(fx, n_in, (const int*)(w.up + p->o_st), (const float*)(w.up + p->o_fr), n, Np, dpcm, st);
    } else {  // convert + polyphase rule + zero padding in one launch
      voice_ingest(w.up, p->s16, n_in, (const float*)(w.up + p->o_taps), p->rp, n, Np, dpcm, st);
    }
    PTTS_HIP(hipGetLastError());
    std::vector<Op> ops;
    float *A = w.A, *Bf = w.Bf, *V = w.V, *zeros = w.zeros;
    {
      const float *wt = W(L_.ec0_w), *b = W(L_.ec0_b);
      ops.push_back({"enc.conv0", [=](hipStream_t s) { conv_cin1(dpcm, Np, 64, 7, wt, b, A, s); }});
    }
    int T = Np, ch = 64;
    for (int i = 0; i < 3; ++i) {
      const int r = RATIOS[2 - i];
      conv_op(ops, "enc.res_conv3", A, 1, T, ch, zeros, 2, 1, 1, W(L_.era_w[i]), ch / 2, 3, 1, W(L_.era_b[i]),
              nullptr, V, T, 1);
      conv_op(ops, "enc.res_conv1", V, 1, T, ch / 2, nullptr, 0, 1, 1, W(L_.erb_w[i]), ch, 1, 1, W(L_.erb_b[i]), A,
              Bf, T, 1);
      conv_op(ops, "enc.down", Bf, 1, T, ch, zeros, r, r, 1, W(L_.edn_w[i]), 2 * ch, 2 * r, 1, W(L_.edn_b[i]),
              nullptr, A, T / r, 1);
      T /= r;
      ch *= 2;
    }
    conv_op(ops, "enc.conv_final", A, 1, T, 512, zeros, 2, 1, 1, W(L_.efin_w), 512, 3, 1, W(L_.efin_b), nullptr, Bf,
            T, 1);
    encoder_transformer(ops, Bf, Te, w.eh, w.eqkv, w.eq, w.eo, w.eu, w.ering);  // on Bf rows [Te][512]
    // ConvDownsample1d k32 s16 per chunk of cf frames, each with the replicate padding of its first
    // frame: one launch writes every chunk's replicated first row, full chunks run as one batched
    // implicit GEMM (chunk = batch row, history = that chunk's rows), a shorter last chunk as a
    // second launch.
    const int nfull = F / cf, rem = F - nfull * cf, nch = nfull + (rem ? 1 : 0);
    float *Hd = w.Hd, *lat = w.lat;
    ops.push_back({"enc.replicate", [=](hipStream_t s) { replicate_chunks(Bf, (long)cf * 16 * 512, Hd, nch, 16, 512, s); }});
    if (nfull)
      conv_op(ops, "enc.downsample", Bf, nfull, cf * 16, 512, Hd, 16, 16, 0, W(L_.down_w), 512, 32, 1, nullptr,
              nullptr, lat, cf, 1);
    if (rem)
      conv_op(ops, "enc.downsample", Bf + (size_t)nfull * cf * 16 * 512, 1, rem * 16, 512,
              Hd + (size_t)nfull * 16 * 512, 16, 16, 0, W(L_.down_w), 512, 32, 1, nullptr, nullptr,
              lat + (size_t)nfull * cf * 512, rem, 1);
    dense_op(ops, "enc.speaker_proj", lat, F, W(L_.speaker_proj), D, MD, nullptr, ACT_NONE, nullptr, nullptr, w.cond);
    run_ops_on(ops, st);
    if (h_cond)  // ahead of the prefill, which turns the rows into the residual stream in place
      PTTS_HIP(hipMemcpyAsync(h_cond, w.cond, sizeof(float) * (size_t)F * D, hipMemcpyDeviceToHost, st));
  }
  for (int c0 = 0; c0 < F; c0 += PREFILL) {
    const int T = std::min(PREFILL, F - c0);
    FlowBufs b = w.fb;
    b.x = w.fb.x + (size_t)c0 * D;
    b.kv = KvStore{v->kv, 0, F};  // the voice's own compact cache [NL][2][NH][F][64]
    b.kv_layer = (long)2 * NH * F * 64;
    std::vector<Op> ops;
    prefill_rows(ops, 0, T, c0, b);
    run_ops_on(ops, st);
  }
  if (v->ev) PTTS_HIP(hipEventRecord(v->ev, st));
}

// The synchronous call: p (and the caller's samples `src`), or p == nullptr and F prompt rows `src`.
ptts_voice* Engine::voice_sync(const VoicePlan* p, const void* src, int F) {
  sync();
  VoiceWs w;  // transient, sized to this clip; vws_ and its pending jobs are not touched
  ptts_voice* v = nullptr;
  try {
    vws_reserve(w, stream_, F, 0, p ? p->dev_bytes : 0);
    v = voice_new(F, p != nullptr, false);
    auto up = [&](void* dst, const void* from, size_t bytes) {
      if (bytes) PTTS_HIP(hipMemcpyAsync(dst, from, bytes, hipMemcpyHostToDevice, stream_));
    };
    if (p) {  // the pieces of a job's single upload, from the caller's memory and the plan's
      up(w.up, src, (size_t)p->n_in * (p->s16 ? 2 : 4));
      up(w.up + p->o_taps, p->taps.data(), p->taps.size() * sizeof(float));
      up(w.up + p->o_st, p->sst.data(), p->sst.size() * sizeof(int));
      up(w.up + p->o_fr, p->sfr.data(), p->sfr.size() * sizeof(float));
    } else {
      up(w.fb.x, src, sizeof(float) * (size_t)F * D);
    }
    voice_clone(p, w, stream_, v, p ? v->cond.data() : nullptr);
    PTTS_HIP(hipStreamSynchronize(stream_));
  } catch (...) {
    (void)hipStreamSynchronize(stream_);
    vws_free(w);
    if (v) free_voice(v);
    throw;
  }
  vws_free(w);
  return v;
}

ptts_voice* Engine::voice_from_prompt(const float* prompt, int F) {
  PTTS_REQUIRE(ready_, "engine weights not finalized");
  PTTS_REQUIRE(prompt != nullptr && F >= 1, "empty prompt");
  PTTS_REQUIRE(F < max_ctx_, "prompt longer than max_ctx");
  return voice_sync(nullptr, prompt, F);
}

ptts_voice* Engine::voice_from_audio(const float* pcm_in, int n_in, int sr, int chunk_frames, int resampler) {
  PTTS_REQUIRE(ready_, "engine weights not finalized");
  PTTS_REQUIRE(pcm_in != nullptr, "empty PCM");
  const VoicePlan p = voice_plan(n_in, PTTS_SAMPLES_F32, sr, chunk_frames, resampler, max_ctx_);
  return voice_sync(&p, pcm_in, p.F);
}

// The job: p and the samples, or p == nullptr and F prompt rows, uploaded through a pinned block
ptts_voice* Engine::voice_job(const VoicePlan* p, const void* src, int F) {
  const size_t bytes = p ? p->up_bytes : sizeof(float) * (size_t)F * D;
  vjob_reserve(F, bytes, p ? p->dev_bytes : 0);
  ptts_voice* v = voice_new(F, p != nullptr, true);
  try {
    VoiceWs& w = vws_;
    const int par = (int)(vjobs_ & 1);
    PTTS_HIP(hipEventSynchronize(w.ev_up[par]));  // the staging block's previous upload (two jobs back)
    char* hs = w.h_up[par];
    memcpy(hs, src, p ? (size_t)p->n_in * (p->s16 ? 2 : 4) : bytes);
    if (p && !p->taps.empty()) memcpy(hs + p->o_taps, p->taps.data(), p->taps.size() * sizeof(float));
    if (p && !p->sst.empty()) memcpy(hs + p->o_st, p->sst.data(), p->sst.size() * sizeof(int));
    if (p && !p->sfr.empty()) memcpy(hs + p->o_fr, p->sfr.data(), p->sfr.size() * sizeof(float));
    // a prompt's rows go straight into x
    PTTS_HIP(hipMemcpyAsync(p ? (void*)w.up : (void*)w.fb.x, hs, bytes, hipMemcpyHostToDevice, stream_vc_));
    PTTS_HIP(hipEventRecord(w.ev_up[par], stream_vc_));
    ++vjobs_;
    voice_clone(p, w, stream_vc_, v, v->h_cond);
  } catch (...) {
    (void)hipStreamSynchronize(stream_vc_);
    free_voice(v);
    throw;
  }
  return v;
}

// vws_ holds `frames` frames and the two block sizes; the voice stream exists
void Engine::vjob_reserve(int frames, size_t host_bytes, size_t up_bytes) {
  PTTS_HIP(hipSetDevice(dev_));
  if (!stream_vc_) {
    int least = 0, greatest = 0;
    PTTS_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    PTTS_HIP(hipStreamCreateWithPriority(&stream_vc_, hipStreamNonBlocking, least));
    for (hipEvent_t& e : vws_.ev_up) PTTS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  vws_reserve(vws_, stream_vc_, std::max(frames, vws_.frames), host_bytes, up_bytes);
}

void Engine::voice_jobs_reserve(int max_frames) {
  PTTS_REQUIRE(ready_, "engine weights not finalized");
  PTTS_REQUIRE(max_frames >= 1 && max_frames < max_ctx_, "max_frames must be in [1, max_ctx)");
  // uploads of float32 clips at up to twice the model's rate, plus the resampler's tables
  const size_t up = al16((size_t)max_frames * FRAME * 2 * sizeof(float)) + (64 << 10);
  vjob_reserve(max_frames, up, up);
}

ptts_voice* Engine::voice_job_prompt(const float* prompt, int F) {
  PTTS_REQUIRE(ready_, "engine weights not finalized");
  PTTS_REQUIRE(prompt != nullptr && F >= 1, "empty prompt");
  PTTS_REQUIRE(F < max_ctx_, "prompt longer than max_ctx");
  return voice_job(nullptr, prompt, F);
}

ptts_voice* Engine::voice_job_audio(const void* samples, int n_in, int fmt, int sr, int chunk_frames, int resampler) {
  PTTS_REQUIRE(ready_, "engine weights not finalized");
  PTTS_REQUIRE(samples != nullptr, "empty PCM");
  const VoicePlan p = voice_plan(n_in, fmt, sr, chunk_frames, resampler, max_ctx_);
  return voice_job(&p, samples, p.F);
}

void Engine::slot_open(int slot, const ptts_voice* v, const int32_t* ids, int n, const ptts_gen_params& p,
                       int lsd_steps) {
  ptts_slot_opts o{};
  o.lsd_steps = lsd_steps;
  slots_open(1, &slot, &v, ids, &n, &p, &o);
}

// Euler steps of a front part over rows [0, B): the largest per-row count among the rows the
// host still holds open (admitted, and neither closed nor seen finished by fetch()). A row that has
// finished on the device but is not yet drained here only costs time; a row that may still be
// active is never given fewer steps than its own count. No open row: the engine's default.
int Engine::lsd_run_for(int B) const {
  int run = 0;
  for (int b = 0; b < B; ++b)
    if (!drained_[b]) run = std::max(run, slot_lsd_[b]);
  return run > 0 ? run : lsd_;
}

// Batched admission: the per-segment prologue of generate_stream_segment (tts_model.rs:938-1004)
// for n utterances at once. Voice KV prefixes are copied in (copy-on-admit, tts_model.rs:940),
// Mimi/conv state reset, and all utterances' text tokens are prefilled together: rows are laid out
// per slot, padded to 16-row groups (the 16-query attention tiles), and mapped to (slot, position)
// through a row table.
void Engine::slots_open(int n, const int* slots, const ptts_voice* const* voices, const int32_t* ids,
                        const int* n_ids, const ptts_gen_params* params, const ptts_slot_opts* opts) {
  PTTS_REQUIRE(ready_, "engine weights not finalized");
  PTTS_REQUIRE(n >= 1 && n <= max_slots_, "number of admissions out of range");
  PTTS_REQUIRE(slots && voices && n_ids && params, "null argument");
  // What a row's options come to: checked, and in the units the tables and the reset kernel take
  struct Row {
    int lsd = 0;                    // Euler steps
    int wfmt = 0;                   // wire format (encoding | rate index << 8; 0: none)
    int speed = 0;                  // WSOLA speed (permille; 0: none)
    unsigned pitch = 0;             // pitch step (Q20; 0: none)
    unsigned gain = 0;              // gain (f32 bits; 0: not in the level stage)
    const float* prefix = nullptr;  // latent prefix and its frames (section 20)
    int npre = 0;
    int reset = 0;                  // RESET_* bits
    int align = 0;                  // text tokens in the align stage (0: the row is not in it)
    int loud = 0;                   // 1: the row is metered (section 27)
  };
  const auto plan = [&](const ptts_slot_opts& o, const ptts_voice* v, int nid, const ptts_gen_params& p) {
    Row r;
    PTTS_REQUIRE(o.align == 0 || o.align == 1, "align must be 0 or 1");
    if (o.align) {  // section 26
      PTTS_REQUIRE(align_, "align needs an align-enabled engine (ptts_align_enable before the first step)");
      PTTS_REQUIRE(nid <= ALIGN_TOKENS, "align: more than PTTS_ALIGN_TOKENS token ids");
    }
    const int sp = o.speed_permille;
    if (sp != 0 && sp != 1000) {  // 1000: no tempo stage for the row, like no speed at all
      PTTS_REQUIRE(sp >= TEMPO_SP_MIN && sp <= TEMPO_SP_MAX, "speed_permille must be 0 or in [500, 2000]");
      PTTS_REQUIRE(tempo_, "a speed needs a tempo-enabled engine (ptts_tempo_enable before the first step)");
      r.speed = sp;
    }
    const int cents = o.pitch_cents;
    if (cents != 0) {  // the WSOLA stage runs at sp_w, the resampler at step (section 23)
      PTTS_REQUIRE(cents >= -PITCH_CENTS_MAX && cents <= PITCH_CENTS_MAX, "pitch_cents must be in [-1200, 1200]");
      PTTS_REQUIRE(pitch_, "a pitch needs a pitch-enabled engine (ptts_pitch_enable before the first step)");
      int sp_w = 0;
      PTTS_REQUIRE(pitch_plan(cents, sp, &sp_w, &r.pitch),
                   "pitch_cents with this speed leaves the time-scaling range (speed / 2^(cents / 1200) in [0.5, 2.0])");
      r.speed = sp_w == 1000 ? 0 : sp_w;
    }
    const int gdb = o.gain_cdb, lim = o.limit;
    PTTS_REQUIRE(gdb >= -LEVEL_GAIN_CDB_MAX && gdb <= LEVEL_GAIN_CDB_MAX, "gain_cdb must be in [-2400, 2400]");
    PTTS_REQUIRE(lim == 0 || lim == 1, "limit must be 0 or 1");
    if (gdb != 0 || lim == 1) {  // the row is in the level stage (section 24)
      PTTS_REQUIRE(level_, "a gain or limit needs a level-enabled engine (ptts_level_enable before the first step)");
      float g = 1.f;
      level_plan(gdb, 0, &g, nullptr);
      memcpy(&r.gain, &g, sizeof g);
    }
    PTTS_REQUIRE(o.loud == 0 || o.loud == 1, "loud must be 0 or 1");
    if (o.loud) {  // section 27
      PTTS_REQUIRE(loud_, "loud needs a loudness-enabled engine (ptts_loud_enable before the first step)");
      r.loud = 1;
    }
    const int wr = o.wire_rate, we = o.wire_encoding;
    if (wr || we || r.speed || r.pitch || r.gain || r.loud) {  // a speed, a pitch, a gain or a meter with no format: 24000 / 16 bit
      PTTS_REQUIRE(wire_, "a wire format needs a wire-enabled engine (ptts_wire_enable before the first step)");
      const int ri = wire_rate_index(wr ? wr : PTTS_SAMPLE_RATE);
      PTTS_REQUIRE(ri >= 0, "wire_rate must be 0 (24000) or one of 8000, 16000, 24000, 44100, 48000");
      PTTS_REQUIRE(we != WIRE_FLAC || flac_, "PTTS_WIRE_FLAC needs a FLAC-enabled engine (ptts_flac_enable before the first step)");
      PTTS_REQUIRE(we >= 0 && we <= WIRE_FLAC, "wire_encoding must be 0 (s16) or PTTS_WIRE_S16 / _ULAW / _ALAW / _FLAC");
      r.wfmt = (we ? we : WIRE_S16) | ri << 8;
    }
    PTTS_REQUIRE(v != nullptr && v->owner == this, "voice belongs to another engine");
    PTTS_REQUIRE(nid >= 0 && (nid == 0 || ids != nullptr), "bad token ids");
    PTTS_REQUIRE(p.max_frames >= 1, "max_frames must be >= 1");
    // 0: the engine's default (its cap)
    PTTS_REQUIRE(o.lsd_steps == 0 || (o.lsd_steps >= 1 && o.lsd_steps <= lsd_),
                 "lsd_steps must be 0 (the default) or in [1, " + std::to_string(lsd_) + "] (the engine's lsd_decode_steps)");
    PTTS_REQUIRE(p.frames_after_eos >= 0, "frames_after_eos must be >= 0");
    PTTS_REQUIRE(o.n_prefix >= 0, "n_prefix must be >= 0");
    PTTS_REQUIRE(o.n_prefix == 0 || o.prefix_latents, "n_prefix > 0 with no prefix_latents");
    PTTS_REQUIRE(o.keep_codec == 0 || o.keep_codec == 1, "keep_codec must be 0 or 1");
    PTTS_REQUIRE((long)v->F + nid + o.n_prefix + p.max_frames <= max_ctx_,
                 o.n_prefix ? "voice + text + prefix + max_frames exceeds max_ctx" : "voice + text + max_frames exceeds max_ctx");
    r.lsd = o.lsd_steps ? o.lsd_steps : lsd_;
    r.prefix = o.prefix_latents;
    r.npre = o.n_prefix;
    r.reset = (o.keep_codec ? RESET_KEEP_CODEC : 0) | (o.n_prefix ? RESET_LAT_SRC : 0);
    r.align = o.align ? nid : 0;
    return r;
  };
  std::vector<char> seen(max_slots_, 0);
  std::vector<Row> row(n);
  bool any_prefix = false, any_opt = false;
  long total_ids = 0;
  for (int i = 0; i < n; ++i) {  // nothing is admitted when one row is refused
    const int slot = slots[i];
    PTTS_REQUIRE(slot >= 0 && slot < max_slots_, "slot out of range");
    PTTS_REQUIRE(!seen[slot], "slot admitted twice in one call");
    seen[slot] = 1;
    row[i] = plan(opts ? opts[i] : ptts_slot_opts{}, voices[i], n_ids[i], params[i]);
    any_prefix = any_prefix || row[i].npre > 0;
    any_opt = any_opt || row[i].reset != 0;
    for (int j = 0; j < n_ids[i]; ++j)
      PTTS_REQUIRE(ids[total_ids + j] >= 0 && ids[total_ids + j] < VOCAB, "token id out of range");
    total_ids += n_ids[i];
  }
  // keep_codec: the slot's codec state must be that of a whole utterance, with nothing in flight
  for (int i = 0; i < n; ++i)
    if ((row[i].reset & RESET_KEEP_CODEC) && !(drained_[slots[i]] && codec_ok_[slots[i]]))
      throw Error(PTTS_ERR_STATE, "keep_codec: the slot's previous utterance was closed or cancelled, or its last "
                                  "frame is not fetched yet");
  // Stream-ordered admission (no drain of the pipeline: a full sync() here stalled the front part
  // at every admission, a large share of the serving path's time): the host waits only until the
  // previous admission has consumed the pinned staging buffers (its event), and stream_ waits on
  // the GPU for the back parts already queued on stream_be_ (which may still decode a frame of a
  // slot's previous utterance: they write its histories and Mimi position) only before the reset
  // of that state, after the text prefill.
  PTTS_HIP(hipEventSynchronize(ev_admit_));
  PTTS_HIP(hipEventSynchronize(ev_act_));  // pending start-of-utterance copies read h_act_
  // voices whose job (voice_job_*) may still run: the front stream waits for the job's event on the
  // GPU, ahead of everything below that reads the prefix; the host does not wait
  for (int i = 0; i < n; ++i) {
    const ptts_voice* v = voices[i];
    if (!v->ev || v->ordered) continue;
    if (hipEventQuery(v->ev) != hipSuccess) PTTS_HIP(hipStreamWaitEvent(stream_, v->ev, 0));
    v->ordered = true;
  }
  if (share_voice_) {
    // shared voice prefixes: each slot's positions < F read the voice's own cache (no copy; the
    // reference copies the prompt's ModelState per utterance, tts_model.rs:940: same values)
    {
      std::lock_guard<std::mutex> lk(voice_mu());
      for (int i = 0; i < n; ++i) ++voices[i]->refs;
    }
    for (int i = 0; i < n; ++i) voice_release(slots[i], false);
    for (int i = 0; i < n; ++i) {
      slot_voice_[slots[i]] = voices[i];
      h_vpre_[slots[i]] = voices[i]->kv;
      h_vlen_[slots[i]] = voices[i]->F;
    }
    // the tables are read by the text prefill below and by the steps after it (stream order); the
    // steps queued before still read the old entries (a freed voice waited for them above)
    PTTS_HIP(hipMemcpyAsync(vpre_, h_vpre_, sizeof(float*) * max_slots_, hipMemcpyHostToDevice, stream_));
    PTTS_HIP(hipMemcpyAsync(vlen_, h_vlen_, sizeof(int) * max_slots_, hipMemcpyHostToDevice, stream_));
  } else {
    // copy-on-admit of the immutable voice prefixes
    for (int i = 0; i < n; ++i) {
      const ptts_voice* v = voices[i];
      PTTS_HIP(hipMemcpy2DAsync(fbm_.kv.base + (size_t)slots[i] * fbm_.kv.slot_stride, sizeof(float) * max_ctx_ * 64, v->kv,
                                sizeof(float) * v->F * 64, sizeof(float) * v->F * 64, NL * 2 * NH,
                                hipMemcpyDeviceToDevice, stream_));
    }
  }
  // text prefill (tts_model.rs:947-964) of every admitted utterance in shared passes
  // a row's latent prefix follows its text, at positions F + S + j: inputs bos, p[0] .. p[n_prefix - 2]
  // (rid: PREFILL_SRC_BOS, then PREFILL_SRC_LAT0 - j; rlat: where latent j lies in the caller's memory)
  std::vector<int> tab, rid;
  std::vector<const float*> rlat;
  long off = 0;
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < n_ids[i]; ++j) {
      tab.push_back(slots[i] << 16 | (voices[i]->F + j));
      rid.push_back(ids[off + j]);
    }
    for (int j = 0; j < row[i].npre; ++j) {
      tab.push_back(slots[i] << 16 | (voices[i]->F + n_ids[i] + j));
      rid.push_back(j == 0 ? PREFILL_SRC_BOS : PREFILL_SRC_LAT0);
      rlat.resize(tab.size(), nullptr);
      if (j > 0) rlat.back() = row[i].prefix + (size_t)(j - 1) * LDIM;
    }
    while (tab.size() % 16) {
      tab.push_back(-1);
      rid.push_back(0);
    }
    off += n_ids[i];
  }
  // The GEMMs, reduces and RoPE run on the tokens only (Tc compact rows: 40 tokens are 40 rows, not
  // 48); the attention keeps the slot-aligned 16-row groups (RowMap::ptab / qrow / orow)
  for (size_t c0 = 0; c0 < tab.size(); c0 += PREFILL) {
    const int T = (int)std::min<size_t>(PREFILL, tab.size() - c0);  // PREFILL % 16 == 0
    if (c0 > 0) PTTS_HIP(hipStreamSynchronize(stream_));  // ids / row table / staging reused by this pass
    int* h_ptab = h_tab_;
    int* h_ctab = h_tab_ + PREFILL;
    int* h_qrow = h_tab_ + 2 * PREFILL;
    int* h_orow = h_tab_ + 3 * PREFILL;
    int Tc = 0, nlat = 0;
    for (int r = 0; r < T; ++r) {
      const int v = tab[c0 + r];
      h_ptab[r] = v;
      h_orow[r] = v < 0 ? -1 : Tc;
      if (v >= 0) {
        h_ctab[Tc] = v;
        h_qrow[Tc] = r;
        h_ids_[Tc] = rid[c0 + r];
        if (c0 + r < rlat.size() && rlat[c0 + r]) {  // staged for this pass (at most T <= PREFILL latents)
          memcpy(h_plat_ + (size_t)nlat * LDIM, rlat[c0 + r], sizeof(float) * LDIM);
          h_ids_[Tc] = PREFILL_SRC_LAT0 - nlat++;
        }
        ++Tc;
      }
    }
    if (Tc == 0) continue;
    if (nlat)
      PTTS_HIP(hipMemcpyAsync(plat_dev_, h_plat_, sizeof(float) * nlat * LDIM, hipMemcpyHostToDevice, stream_));
    PTTS_HIP(hipMemcpyAsync(ids_dev_, h_ids_, sizeof(int) * Tc, hipMemcpyHostToDevice, stream_));
    PTTS_HIP(hipMemcpyAsync(rowtab_dev_, h_ptab, sizeof(int) * T, hipMemcpyHostToDevice, stream_));
    PTTS_HIP(hipMemcpyAsync(ctab_dev_, h_ctab, sizeof(int) * Tc, hipMemcpyHostToDevice, stream_));
    PTTS_HIP(hipMemcpyAsync(qrow_dev_, h_qrow, sizeof(int) * Tc, hipMemcpyHostToDevice, stream_));
    PTTS_HIP(hipMemcpyAsync(orow_dev_, h_orow, sizeof(int) * T, hipMemcpyHostToDevice, stream_));
    std::vector<Op> ops;
    {
      const int* idp = ids_dev_;
      const float* tb = W(L_.embed);
      float* x = fbm_.x;
      if (any_prefix) {  // token and latent rows in one launch
        const float *pl = plat_dev_, *bos = W(L_.bos), *wt = inw_t_;
        ops.push_back({"prefill.input", [=](hipStream_t s) { prefill_input(idp, Tc, tb, pl, bos, wt, D, x, s); }});
      } else {
        ops.push_back({"prefill.embed", [=](hipStream_t s) { embed_gather(idp, Tc, tb, D, x, s); }});
      }
    }
    {
      float *x = fbm_.x, *h = fbm_.h;
      const float* w = W(L_.fl[0].n1w);
      const float* b = W(L_.fl[0].n1b);
      ops.push_back({"prefill.ln1", [=](hipStream_t s) { layernorm(x, D, h, D, Tc, D, w, b, 1e-5f, s); }});
    }
    RowMap map{0, 1, 0, nullptr, ctab_dev_};
    map.ptab = rowtab_dev_;
    map.mpad = T;
    map.qrow = qrow_dev_;
    map.orow = orow_dev_;
    flow_layers(ops, Tc, map, false, false, "prefill", fbm_);
    run_ops(ops);
  }
  // the slot state the back part owns (Mimi ring position, conv and overlap-add histories, frame
  // flags) is reset only after the back parts already queued, which may still decode the slot's
  // previous utterance; the voice-KV copy and the text prefill above touch front-owned state
  // only, so they run ahead of that wait, beside those back parts
  // That wait is needed only while an admitted slot may still have a frame in flight: a slot whose
  // utterance is drained (never admitted, closed, or its last frame fetched) is written by no
  // queued back part (the commit and the histories touch rows with a frame only), so the front
  // stream does not stall behind the queued back passes at such an admission (the server's case)
  bool drained = true;
  for (int i = 0; i < n; ++i) drained = drained && drained_[slots[i]];
  if (!drained) {
    PTTS_HIP(hipEventRecord(ev_be_tail_, stream_be_));
    PTTS_HIP(hipStreamWaitEvent(stream_, ev_be_tail_, 0));
  }
  for (int i = 0; i < n; ++i) {
    drained_[slots[i]] = 0;
    codec_ok_[slots[i]] = 0;
    cancelled_[slots[i]] = 0;
    admit_call_[slots[i]] = k_;
    slot_lsd_[slots[i]] = row[i].lsd;
    if (wire_) slot_wire_[slots[i]] = row[i].wfmt;
  }
  if (tempo_) {
    for (int i = 0; i < n; ++i) h_tempo_[i] = row[i].speed;
    PTTS_HIP(hipMemcpyAsync(admit_tempo_, h_tempo_, sizeof(int) * n, hipMemcpyHostToDevice, stream_));
  }
  if (pitch_) {
    for (int i = 0; i < n; ++i) h_pitch_[i] = row[i].pitch;
    PTTS_HIP(hipMemcpyAsync(admit_pitch_, h_pitch_, sizeof(unsigned) * n, hipMemcpyHostToDevice, stream_));
  }
  if (level_) {
    for (int i = 0; i < n; ++i) h_level_[i] = row[i].gain;
    PTTS_HIP(hipMemcpyAsync(admit_level_, h_level_, sizeof(unsigned) * n, hipMemcpyHostToDevice, stream_));
  }
  if (loud_) {
    for (int i = 0; i < n; ++i) h_loud_[i] = row[i].loud;
    PTTS_HIP(hipMemcpyAsync(admit_loud_, h_loud_, sizeof(int) * n, hipMemcpyHostToDevice, stream_));
  }
  // fresh Mimi decoder state (init_states(1, 1000) per segment, tts_model.rs:941) + slot states
  std::vector<SlotState> st(n);
  std::vector<int> fp(n);
  for (int i = 0; i < n; ++i) {
    const ptts_gen_params& p = params[i];
    SlotState& s = st[i];
    s = SlotState{};
    s.active = 1;
    s.step = 0;
    s.eos_step = -1;
    s.frames_after_eos = p.frames_after_eos;
    s.max_frames = p.max_frames;
    s.temp = p.temp;
    s.eos_threshold = p.eos_threshold;
    s.noise_clamp = p.noise_clamp;
    s.seed = p.seed;
    s.lsd = slot_lsd_[slots[i]];
    fp[i] = voices[i]->F + n_ids[i] + row[i].npre;
  }
  // staged through pinned buffers so the copies are truly asynchronous: admission returns with
  // the prefill still running and the caller's first step queued right behind it (no host
  // round trip in between); the event wait above guarantees the staging is free again
  // multi-frame passes: an utterance's frames group into passes from its first, so rows admitted
  // inside a pass stay inactive for the pass's remaining calls and start at the next pass (their
  // state is written then)
  admit_delay_ = nfr_ > 1 ? (int)((nfr_ - k_ % nfr_) % nfr_) : 0;
  if (admit_delay_)
    for (int i = 0; i < n; ++i) {
      h_act_[slots[i]] = st[i];
      act_slots_.push_back(slots[i]);
      st[i].active = 0;
    }
  // first-frame previews: each admitted row's first front part runs at call k_ + admit_delay_ (a
  // re-admitted slot's unfetched preview belonged to its previous utterance)
  for (int i = 0; i < n; ++i) pv_forget(slots[i]);
  // (a preview decodes from the fresh codec state: not the frame a keep_codec row produces)
  if (pv_max_ > 0)
    for (int i = 0; i < n; ++i)
      if (!(row[i].reset & RESET_KEEP_CODEC)) pv_pending_.push_back({slots[i], k_ + admit_delay_});
  memcpy(h_slots_, slots, sizeof(int) * n);
  memcpy(h_st_, st.data(), sizeof(SlotState) * n);
  memcpy(h_fp_, fp.data(), sizeof(int) * n);
  if (wire_) {
    for (int i = 0; i < n; ++i) h_wire_[i] = row[i].wfmt;
    PTTS_HIP(hipMemcpyAsync(admit_wire_, h_wire_, sizeof(int) * n, hipMemcpyHostToDevice, stream_));
  }
  PTTS_HIP(hipMemcpyAsync(admit_slots_, h_slots_, sizeof(int) * n, hipMemcpyHostToDevice, stream_));
  PTTS_HIP(hipMemcpyAsync(admit_st_, h_st_, sizeof(SlotState) * n, hipMemcpyHostToDevice, stream_));
  PTTS_HIP(hipMemcpyAsync(admit_fpos_, h_fp_, sizeof(int) * n, hipMemcpyHostToDevice, stream_));
  if (align_) {
    // the rows' {first text position, tokens}: front-owned like fpos_, written on the front stream
    // behind the front parts already issued and ahead of the row's first; from the admission's
    // pinned staging (free again: ev_admit_ above). Only entries that change are written, so an
    // engine whose rows never ask for alignment enqueues nothing here.
    for (int i = 0; i < n; ++i) {
      const int na = row[i].align;
      if (!na && !slot_align_[slots[i]]) continue;
      h_align_src_[i] = AlignEntry{voices[i]->F, na};
      PTTS_HIP(hipMemcpyAsync(align_tab_ + slots[i], h_align_src_ + i, sizeof(AlignEntry), hipMemcpyHostToDevice,
                              stream_));
      slot_align_[slots[i]] = na;
    }
  }
  if (any_opt) {  // the rows' first backbone input (the prefix's last latent) and RESET_* bits
    for (int i = 0; i < n; ++i) {
      h_aopt_[i] = row[i].reset;
      if (row[i].npre)
        memcpy(h_alat_ + (size_t)i * LDIM, row[i].prefix + (size_t)(row[i].npre - 1) * LDIM, sizeof(float) * LDIM);
    }
    PTTS_HIP(hipMemcpyAsync(admit_opt_, h_aopt_, sizeof(int) * n, hipMemcpyHostToDevice, stream_));
    if (any_prefix)
      PTTS_HIP(hipMemcpyAsync(admit_lat_, h_alat_, sizeof(float) * n * LDIM, hipMemcpyHostToDevice, stream_));
  }
  {
    ResetArgs r = reset_args(n);
    if (wire_) {  // the wire state is back-owned too: same reset, same ordering
      r.wire_src = admit_wire_;
      r.wire_fmt = wire_fmt_;
      r.wire_frames = wire_frames_;
    }
    if (tempo_) {
      r.tempo_src = admit_tempo_;
      r.tempo_sp = tempo_sp_;
      r.tempo_state = tempo_state_;
    }
    if (pitch_) {
      r.pitch_src = admit_pitch_;
      r.pitch_step = pitch_step_;
      r.pitch_state = pitch_state_;
    }
    if (level_) {
      r.level_src = admit_level_;
      r.level_gain = level_gain_;
      r.level_state = level_state_;
    }
    if (loud_) {
      r.loud_src = admit_loud_;
      r.loud_state = loud_state_;
    }
    if (any_opt) {
      r.opt_src = admit_opt_;
      r.lat_src = admit_lat_;
    }
    slot_reset(r, stream_);
    PTTS_HIP(hipGetLastError());
  }
  mark_admission();
  admitted_since_call_ = true;
}

// ------------------------------------------------------------------ wire stage
int Engine::wire_rate_index(int rate) {
  for (int r = 0; r < WIRE_RATES; ++r)
    if (WIRE_RATE_HZ[r] == rate) return r;
  return -1;
}

long Engine::wire_len(long n_samples, int rate, int enc) {
  if (n_samples < 0 || wire_rate_index(rate) < 0 || enc < WIRE_S16 || enc > WIRE_ALAW) return -1;
  return resample_plan(PTTS_SAMPLE_RATE, rate).out_len(n_samples) * (enc == WIRE_S16 ? 2 : 1);
}

void Engine::wire_enable(bool on) {
  PTTS_REQUIRE(k_ == 0 && graphs_.empty(), "wire output is chosen on an idle engine before its first step");
  PTTS_HIP(hipSetDevice(dev_));
  if (on && !wire_fmt_) {
    const size_t B = max_slots_;
    wire_fmt_ = (int*)dalloc(B);
    slot_wire_.assign(B, 0);
    wire_frames_ = (int*)dalloc(B);
    admit_wire_ = (int*)dalloc(B);
    wire_tail_ = dalloc(B * WIRE_TAIL);
    h_wire_ = (int*)halloc(sizeof(int) * B);
    std::vector<float> taps;
    for (int r = 0; r < WIRE_RATES; ++r) {
      const ResamplePlan rp = resample_plan(PTTS_SAMPLE_RATE, WIRE_RATE_HZ[r]);
      wire_plan_[r] = WirePlan{rp.up, rp.down, rp.half, rp.L, (int)taps.size()};
      if (rp.identity()) continue;
      PTTS_REQUIRE(rp.L <= WIRE_TAPS_MAX && 2 * rp.half <= WIRE_TAIL * rp.up, "wire rate outside the stage's window");
      const std::vector<float> h = resample_taps(rp);
      taps.insert(taps.end(), h.begin(), h.end());
    }
    wire_taps_ = dalloc(taps.size());
    PTTS_HIP(hipMemcpy(wire_taps_, taps.data(), sizeof(float) * taps.size(), hipMemcpyHostToDevice));
    wire_blocks_alloc();
  }
  wire_ = on;
}

void Engine::wire_blocks_alloc() {
  const size_t bytes = wire_block_bytes(max_slots_);
  for (int p = 0; p < WIRE_BLOCKS; ++p) {
    wireb_[p] = (unsigned char*)dalloc((bytes + 3) / 4);
    h_wireb_[p] = (unsigned char*)halloc(bytes);
    memset(h_wireb_[p], 0, wire_head_bytes());
  }
}

void Engine::fetch_wire(int calls_back, int B, unsigned char* out, size_t row_stride, int* n_bytes) {
  PTTS_REQUIRE(wire_, "fetch_wire: the engine has no wire output (ptts_wire_enable)");
  PTTS_REQUIRE(B >= 1 && B <= max_slots_, "n_rows out of range");
  PTTS_REQUIRE(calls_back == 0 || calls_back == 1, "calls_back must be 0 or 1");
  PTTS_REQUIRE(n_bytes != nullptr, "null argument");
  PTTS_REQUIRE(!out || row_stride >= (size_t)wire_chunk_max(),
               level_   ? "row_stride must be >= PTTS_WIRE_CHUNK_MAX_LEVEL on a level-enabled engine"
               : tempo_ ? "row_stride must be >= PTTS_WIRE_CHUNK_MAX_TEMPO on a tempo-enabled engine"
                        : "row_stride must be >= PTTS_WIRE_CHUNK_MAX");
  // the same frame, rows and event as fetch() of that call; no bookkeeping of its own
  const int q = calls_back ? prev_hb_ : out_hb_;
  const int rows = calls_back ? prev_rows_ : out_rows_;
  const long long fk = calls_back ? prev_k_ : out_k_;
  if (pipeline_) PTTS_HIP(hipEventSynchronize(ev_back_[q - q % nfr_]));
  else sync();
  const int n = std::min(B, rows);
  const unsigned char* blk = h_wireb_[nfr_ > 1 ? q / nfr_ : q];
  const int* cnt = (const int*)blk;
  for (int b = 0; b < B; ++b) {
    const int f = q % nfr_;
    int c = b < n ? cnt[(size_t)b * nfr_ + f] : 0;
    if (c && !cancel_wins_.empty() && frame_cancelled(b, fk)) c = 0;  // slots_cancel: no byte of that utterance
    if (c < 0 || c > wire_chunk_max()) throw Error(PTTS_ERR_STATE, "fetch_wire: corrupt chunk size");
    if (c && out) memcpy(out + b * row_stride, blk + wire_head_bytes() + ((size_t)b * nfr_ + f) * wire_chunk_max(), c);
    n_bytes[b] = c;
  }
}

void Engine::wire_encode_host(const float* pcm, int n, int rate, int enc, unsigned char* out) {
  PTTS_REQUIRE(pcm && out && n >= 1, "empty input");
  const long bytes = wire_len(n, rate, enc);
  PTTS_REQUIRE(bytes >= 1, "unknown wire rate or encoding");
  const ResamplePlan rp = resample_plan(PTTS_SAMPLE_RATE, rate);
  const long n_out = rp.out_len(n);
  PTTS_REQUIRE(n_out < (1L << 30), "input too long");
  sync();
  void *dx = nullptr, *dh = nullptr, *dy = nullptr, *dw = nullptr;
  try {
    PTTS_HIP(hipMalloc(&dx, sizeof(float) * n));
    PTTS_HIP(hipMalloc(&dw, (size_t)(bytes + 7) / 8 * 8));
    PTTS_HIP(hipMemcpyAsync(dx, pcm, sizeof(float) * n, hipMemcpyHostToDevice, stream_));
    const float* src = (const float*)dx;
    if (!rp.identity()) {  // the whole-signal kernel ptts_resample runs
      const std::vector<float> taps = resample_taps(rp);
      PTTS_HIP(hipMalloc(&dh, sizeof(float) * taps.size()));
      PTTS_HIP(hipMalloc(&dy, sizeof(float) * n_out));
      PTTS_HIP(hipMemcpy(dh, taps.data(), sizeof(float) * taps.size(), hipMemcpyHostToDevice));
      resample((const float*)dx, n, (const float*)dh, rp, (int)n_out, (int)n_out, (float*)dy, stream_);
      src = (const float*)dy;
    }
    wire_encode(src, n_out, enc, (unsigned char*)dw, stream_);
    PTTS_HIP(hipGetLastError());
    PTTS_HIP(hipMemcpyAsync(out, dw, (size_t)bytes, hipMemcpyDeviceToHost, stream_));
    PTTS_HIP(hipStreamSynchronize(stream_));
  } catch (...) {
    (void)hipStreamSynchronize(stream_);
    (void)hipFree(dx), (void)hipFree(dh), (void)hipFree(dy), (void)hipFree(dw);
    throw;
  }
  (void)hipFree(dx), (void)hipFree(dh), (void)hipFree(dy), (void)hipFree(dw);
}

// ------------------------------------------------------------------ align stage
void Engine::align_enable(bool on, int layer, unsigned head_mask) {
  PTTS_REQUIRE(k_ == 0 && graphs_.empty(), "the align stage is chosen on an idle engine before its first step");
  if (on) {
    PTTS_REQUIRE(layer >= 0 && layer < NL, "align: layer must be in [0, 5]");
    PTTS_REQUIRE((head_mask & ((1u << NH) - 1u)) != 0, "align: head_mask selects none of the 16 heads");
  }
  PTTS_HIP(hipSetDevice(dev_));
  if (on && !align_tab_) {
    static_assert(sizeof(AlignEntry) == 2 * sizeof(float) && ALIGN_TOKENS == PTTS_ALIGN_TOKENS, "align layout");
    const size_t B = max_slots_, words = (size_t)NHB * B * ALIGN_ROW;
    align_tab_ = (AlignEntry*)dalloc(2 * B);
    h_align_src_ = (AlignEntry*)halloc(sizeof(AlignEntry) * B);
    slot_align_.assign(B, 0);
    alignb_ = dalloc(words);
    h_alignb_ = (float*)halloc(sizeof(float) * words);
    memset(h_alignb_, 0, sizeof(float) * words);
  }
  align_ = on;
  if (on) {
    align_layer_ = layer;
    align_mask_ = head_mask & ((1u << NH) - 1u);
  }
}

void Engine::fetch_align(int calls_back, int B, float* out, size_t row_stride, int* n_tokens) {
  PTTS_REQUIRE(align_, "fetch_align: the engine has no align stage (ptts_align_enable)");
  PTTS_REQUIRE(B >= 1 && B <= max_slots_, "n_rows out of range");
  PTTS_REQUIRE(calls_back == 0 || calls_back == 1, "calls_back must be 0 or 1");
  PTTS_REQUIRE(n_tokens != nullptr, "null argument");
  PTTS_REQUIRE(!out || row_stride >= (size_t)ALIGN_TOKENS, "row_stride must be >= PTTS_ALIGN_TOKENS");
  // the same frame, rows and event as fetch() of that call; no bookkeeping of its own
  const int q = calls_back ? prev_hb_ : out_hb_;
  const int rows = calls_back ? prev_rows_ : out_rows_;
  const long long fk = calls_back ? prev_k_ : out_k_;
  if (pipeline_) PTTS_HIP(hipEventSynchronize(ev_back_[q - q % nfr_]));
  else sync();
  const int n = fk >= 0 && align_any_[q] ? std::min(B, rows) : 0;  // (no copy for a buffer without a row in the stage)
  const FrameFlags* hf = (const FrameFlags*)(h_meta_[q] + (size_t)max_slots_ * LDIM);
  const float* blk = h_alignb_ + (size_t)q * max_slots_ * ALIGN_ROW;
  for (int b = 0; b < B; ++b) {
    const float* r = blk + (size_t)b * ALIGN_ROW;
    int c = 0;
    if (b < n && hf[b].valid && (cancel_wins_.empty() || !frame_cancelled(b, fk))) memcpy(&c, r, sizeof c);
    if (c < 0 || c > ALIGN_TOKENS) throw Error(PTTS_ERR_STATE, "fetch_align: corrupt token count");
    if (c && out) memcpy(out + b * row_stride, r + 1, sizeof(float) * c);
    n_tokens[b] = c;
  }
}

// Align test hook: the product launcher align_step on host operands, modelled on test_attention's
// step form (one row per slot: row r is slot r). qkv: dense rows [M][3 nh 64] (S == 0) or S slabs;
// kvh [M][2][nh][cap][64]; pre / pre_len: optional shared prefixes, handed to the launcher as the
// engine hands them (the kernel must not read them); pos [M]; tab [M][2] = {t0, n}; out
// [M][ALIGN_ROW] in and out (a row not in the stage keeps its floats).
void Engine::test_align(int M, int nh, int cap, int S, const float* qkv, const float* kvh, const float* pre,
                        const int* pre_len, const int* pos, const int* tab, unsigned head_mask, float* out) {
  PTTS_REQUIRE(ready_, "engine weights not finalized");
  PTTS_REQUIRE(qkv && kvh && pos && tab && out && (!pre || pre_len), "test_align: bad arguments");
  PTTS_REQUIRE(M >= 1 && M <= 64 && nh >= 1 && nh <= 16 && cap >= 1 && cap <= 65536 && S >= 0 && S <= 16,
               "test_align: bad shape");
  PTTS_REQUIRE((head_mask & ((1u << nh) - 1u)) != 0, "test_align: head_mask selects no head");
  for (int r = 0; r < M; ++r) {
    PTTS_REQUIRE(pos[r] >= 0 && pos[r] <= cap, "test_align: step position past the cache");
    const int t0 = tab[2 * r], n = tab[2 * r + 1];
    PTTS_REQUIRE(n >= 0 && n <= ALIGN_TOKENS && t0 >= 0 && t0 + n <= cap, "test_align: text keys outside the store");
  }
  size_t pre_floats = 0;
  std::vector<size_t> pre_off(M, 0);
  if (pre)
    for (int sl = 0; sl < M; ++sl) {
      PTTS_REQUIRE(pre_len[sl] >= 0 && pre_len[sl] <= cap, "test_align: bad prefix length");
      pre_off[sl] = pre_floats;
      pre_floats += (size_t)2 * nh * pre_len[sl] * 64;
    }
  sync();
  const int d = nh * 64, Sk = std::max(S, 1);
  std::vector<void*> allocs;
  auto release = [&]() {
    for (void* p : allocs) (void)hipFree(p);
  };
  try {
    auto dal = [&](size_t bytes) {
      void* p = nullptr;
      PTTS_HIP(hipMalloc(&p, std::max<size_t>(bytes, 16)));
      allocs.push_back(p);
      return p;
    };
    auto up = [&](const void* src, size_t bytes) {
      void* p = dal(bytes);
      PTTS_HIP(hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, stream_));
      return p;
    };
    AlignArgs a{};
    a.P = (const float*)up(qkv, sizeof(float) * Sk * M * 3 * d);
    a.S = Sk;
    a.M = M;
    a.nh = nh;
    a.pos = (const int*)up(pos, sizeof(int) * M);
    a.kv = KvStore{(float*)up(kvh, sizeof(float) * M * 2 * nh * cap * 64), (long)2 * nh * cap * 64, cap};
    std::vector<const float*> prep(M, nullptr);
    if (pre) {
      const float* dpre = (const float*)up(pre, sizeof(float) * pre_floats);
      for (int sl = 0; sl < M; ++sl) prep[sl] = dpre + pre_off[sl];
      a.kv.pre = (const float* const*)up(prep.data(), sizeof(float*) * M);
      a.kv.pre_len = (const int*)up(pre_len, sizeof(int) * M);
    }
    float* drope = (float*)dal(sizeof(float) * cap * 64);
    rope_table(drope, cap, stream_);
    a.rope = drope;
    a.tab = (const AlignEntry*)up(tab, sizeof(AlignEntry) * M);
    a.head_mask = head_mask;
    a.out = (float*)up(out, sizeof(float) * M * ALIGN_ROW);
    align_step(a, stream_);
    PTTS_HIP(hipGetLastError());
    PTTS_HIP(hipMemcpyAsync(out, a.out, sizeof(float) * M * ALIGN_ROW, hipMemcpyDeviceToHost, stream_));
    PTTS_HIP(hipStreamSynchronize(stream_));
  } catch (...) {
    (void)hipStreamSynchronize(stream_);
    release();
    throw;
  }
  release();
}

// ------------------------------------------------------------------ tempo stage
void Engine::tempo_enable(bool on) {
  PTTS_REQUIRE(k_ == 0 && graphs_.empty(), "the tempo stage is chosen on an idle engine before its first step");
  PTTS_REQUIRE(!on || wire_, "the tempo stage needs a wire-enabled engine (ptts_wire_enable first)");
  PTTS_REQUIRE(on || !pitch_, "the pitch stage needs the tempo stage (ptts_pitch_enable(0) first)");
  // section 19: a pending hop reads nothing older than TEMPO_HIST samples, a chunk fits its slots
  static_assert(TEMPO_R == TEMPO_D + TEMPO_HS + TEMPO_W && 2 * TEMPO_HS == TEMPO_W, "tempo constants");
  const int step_max = (TEMPO_HS * TEMPO_SP_MAX + 999) / 1000, step_min = TEMPO_HS * TEMPO_SP_MIN / 1000;
  const long out_max = std::max<long>((long)(FRAME + TEMPO_R - 1) * 1000 / TEMPO_SP_MIN + 1,
                                      (long)FRAME * 1000 / TEMPO_SP_MIN + TEMPO_HS);
  PTTS_REQUIRE(step_min >= TEMPO_D && TEMPO_HIST >= TEMPO_R + step_max + TEMPO_D - TEMPO_HS && TEMPO_HIST <= FRAME &&
                   out_max <= TEMPO_OUT_MAX && (2L * TEMPO_OUT_MAX + 21) * 2 <= WIRE_CHUNK_MAX_TEMPO,
               "tempo constants violate the history or chunk bounds of DESIGN.md section 19");
  PTTS_HIP(hipSetDevice(dev_));
  if (on && !tempo_sp_) {
    const size_t B = max_slots_;
    tempo_sp_ = (int*)dalloc(B);
    tempo_state_ = (int*)dalloc(B * TEMPO_STATE);
    tempo_hist_ = dalloc(B * TEMPO_HIST);
    tempo_out_ = dalloc(B * nfr_ * TEMPO_OUT_MAX);
    tempo_cnt_ = (int*)dalloc(B * nfr_);
    admit_tempo_ = (int*)dalloc(B);
    h_tempo_ = (int*)halloc(sizeof(int) * B);
    const std::vector<float> w = tempo_window();
    tempo_win_ = dalloc(w.size());
    PTTS_HIP(hipMemcpy(tempo_win_, w.data(), sizeof(float) * w.size(), hipMemcpyHostToDevice));
  }
  if (on != tempo_) {  // the chunk slots change size: new pass blocks (the old ones stay until destruction)
    tempo_ = on;
    PTTS_REQUIRE(!level_ || level_min_chunk() >= 16, "level: a non-last chunk below 16 samples (DESIGN.md section 24)");
    wire_blocks_alloc();
  }
}

void Engine::tempo_host(const float* pcm, int n, int sp, float* out) {
  PTTS_REQUIRE(pcm && out && n >= 1, "empty input");
  PTTS_REQUIRE(sp >= TEMPO_SP_MIN && sp <= TEMPO_SP_MAX, "speed_permille must be in [500, 2000]");
  const long n_out = tempo_len(n, sp);
  PTTS_REQUIRE(n_out < (1L << 30), "input too long");
  sync();
  void *dx = nullptr, *dw = nullptr, *dy = nullptr;
  try {
    const std::vector<float> w = tempo_window();
    PTTS_HIP(hipMalloc(&dx, sizeof(float) * n));
    PTTS_HIP(hipMalloc(&dw, sizeof(float) * w.size()));
    PTTS_HIP(hipMalloc(&dy, sizeof(float) * n_out));
    PTTS_HIP(hipMemcpyAsync(dx, pcm, sizeof(float) * n, hipMemcpyHostToDevice, stream_));
    PTTS_HIP(hipMemcpy(dw, w.data(), sizeof(float) * w.size(), hipMemcpyHostToDevice));
    ptts::tempo((const float*)dx, n, sp, (const float*)dw, (float*)dy, stream_);
    PTTS_HIP(hipGetLastError());
    PTTS_HIP(hipMemcpyAsync(out, dy, sizeof(float) * n_out, hipMemcpyDeviceToHost, stream_));
    PTTS_HIP(hipStreamSynchronize(stream_));
  } catch (...) {
    (void)hipStreamSynchronize(stream_);
    (void)hipFree(dx), (void)hipFree(dw), (void)hipFree(dy);
    throw;
  }
  (void)hipFree(dx), (void)hipFree(dw), (void)hipFree(dy);
}

// ------------------------------------------------------------------ pitch stage
void Engine::pitch_enable(bool on) {
  PTTS_REQUIRE(k_ == 0 && graphs_.empty(), "the pitch stage is chosen on an idle engine before its first step");
  PTTS_REQUIRE(!on || tempo_, "the pitch stage needs a tempo-enabled engine (ptts_tempo_enable first)");
  // section 23: the history covers 2 H inputs, and the largest chunk (a last frame: the tempo stage's
  // last chunk and the H flushed inputs, over step / 2^20) fits PITCH_OUT_MAX, the chunk slot through
  // the 48 kHz resampler, and the FLAC stage's chunk. sp_w grows with the speed: the smallest valid
  // speed of each pitch bounds it.
  long out_max = 0;
  int h_max = 0;
  for (int cents = -PITCH_CENTS_MAX; cents <= PITCH_CENTS_MAX; ++cents) {
    int sp_w = 0;
    unsigned step = 0;
    int sp = TEMPO_SP_MIN;
    while (sp <= TEMPO_SP_MAX && !pitch_plan(cents, sp, &sp_w, &step)) ++sp;
    PTTS_REQUIRE(sp <= TEMPO_SP_MAX, "a pitch with no valid speed");
    const int H = pitch_support(step);
    const long in_max = (long)(FRAME + TEMPO_R - 1) * 1000 / sp_w + 1;  // (a PCM frame at sp_w 1000 is shorter)
    h_max = std::max(h_max, H);
    out_max = std::max(out_max, (((in_max + H) << 20) + step - 1) / step);
  }
  PTTS_REQUIRE(2 * h_max <= PITCH_HIST && out_max <= PITCH_OUT_MAX && 2L * PITCH_OUT_MAX + 21 <= FLAC_CHUNK_SAMPLES &&
                   (2L * PITCH_OUT_MAX + 21) * 2 <= WIRE_CHUNK_MAX_TEMPO,
               "pitch constants violate the history or chunk bounds of DESIGN.md section 23");
  PTTS_HIP(hipSetDevice(dev_));
  if (on && !pitch_step_) {
    const size_t B = max_slots_;
    pitch_step_ = (unsigned*)dalloc(B);
    pitch_state_ = (int*)dalloc(B * PITCH_STATE);
    pitch_hist_ = dalloc(B * PITCH_HIST);
    pitch_out_ = dalloc(B * nfr_ * PITCH_OUT_MAX);
    pitch_cnt_ = (int*)dalloc(B * nfr_);
    admit_pitch_ = (unsigned*)dalloc(B);
    h_pitch_ = (unsigned*)halloc(sizeof(unsigned) * B);
    const std::vector<float> tab = pitch_table();
    pitch_tab_ = dalloc(tab.size());
    PTTS_HIP(hipMemcpy(pitch_tab_, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice));
  }
  pitch_ = on;
  PTTS_REQUIRE(!level_ || level_min_chunk() >= 16, "level: a non-last chunk below 16 samples (DESIGN.md section 24)");
}

void Engine::pitch_host(const float* x, int n, unsigned step, float* y) {
  PTTS_REQUIRE(x && y && n >= 1, "empty input");
  PTTS_REQUIRE(step >= PITCH_STEP_MIN && step <= PITCH_STEP_MAX, "step_q20 must be in [2^19, 2^21]");
  PTTS_REQUIRE(n < (1 << 29), "input too long");
  const long n_out = pitch_len(n, step);
  if (n_out < 1) return;
  sync();
  void *dx = nullptr, *dt = nullptr, *dy = nullptr;
  try {
    const std::vector<float> tab = pitch_table();
    PTTS_HIP(hipMalloc(&dx, sizeof(float) * n));
    PTTS_HIP(hipMalloc(&dt, sizeof(float) * tab.size()));
    PTTS_HIP(hipMalloc(&dy, sizeof(float) * n_out));
    PTTS_HIP(hipMemcpyAsync(dx, x, sizeof(float) * n, hipMemcpyHostToDevice, stream_));
    PTTS_HIP(hipMemcpy(dt, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice));
    ptts::pitch_resample((const float*)dx, n, step, (const float*)dt, (float*)dy, stream_);
    PTTS_HIP(hipGetLastError());
    PTTS_HIP(hipMemcpyAsync(y, dy, sizeof(float) * n_out, hipMemcpyDeviceToHost, stream_));
    PTTS_HIP(hipStreamSynchronize(stream_));
  } catch (...) {
    (void)hipStreamSynchronize(stream_);
    (void)hipFree(dx), (void)hipFree(dt), (void)hipFree(dy);
    throw;
  }
  (void)hipFree(dx), (void)hipFree(dt), (void)hipFree(dy);
}

// ------------------------------------------------------------------ level stage
// The smallest first chunk of a level row at the wire rate, over every valid (speed, pitch, rate) of
// this engine's stages (section 24): the stage delays the row by L samples, so a first chunk is L
// samples shorter than its input's and every later non-last chunk is as long as its input's.
long Engine::level_min_chunk() const {
  long least = 1L << 40;
  auto through = [&](long seen) {  // the first chunk of `seen` inputs of the level stage, at each wire rate
    const long lv = std::max(seen - LEVEL_L, 0L);
    for (int r = 0; r < WIRE_RATES; ++r) {
      const ResamplePlan rp = resample_plan(PTTS_SAMPLE_RATE, WIRE_RATE_HZ[r]);
      least = std::min(least, rp.identity() || lv == 0 ? lv : (lv * rp.up - 1 - rp.half) / rp.down + 1);
    }
  };
  auto tempo_first = [](int sp_w) {  // hops run in the first frame: every k with floor(k Hs sp / 1000) + R <= FRAME
    long k = 0;
    while ((k * TEMPO_HS * sp_w) / 1000 + TEMPO_R <= FRAME) ++k;
    return k * TEMPO_HS;
  };
  through(FRAME);
  if (tempo_)
    for (int sp = TEMPO_SP_MIN; sp <= TEMPO_SP_MAX; ++sp) through(tempo_first(sp));
  if (pitch_)
    for (int cents = -PITCH_CENTS_MAX; cents <= PITCH_CENTS_MAX; ++cents) {
      int lo = TEMPO_SP_MIN, hi = TEMPO_SP_MAX, sp_w = 0;
      unsigned step = 0;
      while (lo <= TEMPO_SP_MAX && !pitch_plan(cents, lo, &sp_w, &step)) ++lo;
      while (hi >= lo && !pitch_plan(cents, hi, &sp_w, &step)) --hi;
      for (int sp : {lo, hi}) {  // sp_w grows with the speed and the first tempo chunk shrinks with sp_w
        if (!pitch_plan(cents, sp, &sp_w, &step)) continue;
        const long t1 = sp_w == 1000 ? FRAME : tempo_first(sp_w), H = pitch_support(step);
        through(t1 > H ? (((t1 - H) << 20) + step - 1) / step : 0);
      }
    }
  return least;
}

void Engine::level_enable(bool on, int ceiling_cdb) {
  PTTS_REQUIRE(k_ == 0 && graphs_.empty(), "the level stage is chosen on an idle engine before its first step");
  PTTS_REQUIRE(!on || wire_, "the level stage needs a wire-enabled engine (ptts_wire_enable first)");
  float ceiling = 1.f;
  PTTS_REQUIRE(!on || level_plan(0, ceiling_cdb, nullptr, &ceiling), "ceiling_cdb must be in [-4000, 0]");
  // section 24: the largest chunk (a last frame: the largest input chunk and the L flushed outputs)
  // fits LEVEL_OUT_MAX, the chunk slot through the 48 kHz resampler (2 n + 20 outputs at most, as in
  // section 19) and the FLAC stage's chunk; a FLAC chunk is at most three frames; a non-last chunk
  // is a legal FLAC block (16 samples at least) at every rate
  const long in_max = std::max<long>(FRAME, std::max(TEMPO_OUT_MAX, PITCH_OUT_MAX)), out_max = in_max + LEVEL_L;
  const long wire_max = 2 * out_max + 21;
  PTTS_REQUIRE(in_max <= LEVEL_IN_MAX && out_max <= LEVEL_OUT_MAX && wire_max <= FLAC_CHUNK_SAMPLES &&
                   wire_max * 2 <= WIRE_CHUNK_MAX_LEVEL && flac_bound(wire_max) <= WIRE_CHUNK_MAX_LEVEL &&
                   wire_max <= 3L * FLAC_BLOCK && LEVEL_HIST + LEVEL_IN_MAX + LEVEL_L <= LEVEL_WINDOW,
               "level constants violate the chunk bounds of DESIGN.md section 24");
  PTTS_REQUIRE(!on || level_min_chunk() >= 16, "level: a non-last chunk below 16 samples (DESIGN.md section 24)");
  PTTS_HIP(hipSetDevice(dev_));
  if (on && !level_gain_) {
    const size_t B = max_slots_;
    level_gain_ = (unsigned*)dalloc(B);
    level_state_ = (int*)dalloc(B * LEVEL_STATE);
    level_hist_ = dalloc(B * LEVEL_HIST);
    level_out_ = dalloc(B * nfr_ * LEVEL_OUT_MAX);
    level_cnt_ = (int*)dalloc(B * nfr_);
    admit_level_ = (unsigned*)dalloc(B);
    h_level_ = (unsigned*)halloc(sizeof(unsigned) * B);
  }
  if (on) level_ceiling_ = ceiling;
  if (on != level_) {  // the chunk slots change size: new pass blocks (the old ones stay until destruction)
    level_ = on;
    wire_blocks_alloc();
  }
}

void Engine::level_host(const float* x, int n, int gain_cdb, int ceiling_cdb, float* y) {
  PTTS_REQUIRE(x && y && n >= 1, "empty input");
  float v = 1.f, c = 1.f;
  PTTS_REQUIRE(level_plan(gain_cdb, ceiling_cdb, &v, &c), "gain_cdb must be in [-2400, 2400], ceiling_cdb in [-4000, 0]");
  sync();
  void *dx = nullptr, *dy = nullptr;
  try {
    PTTS_HIP(hipMalloc(&dx, sizeof(float) * n));
    PTTS_HIP(hipMalloc(&dy, sizeof(float) * n));
    PTTS_HIP(hipMemcpyAsync(dx, x, sizeof(float) * n, hipMemcpyHostToDevice, stream_));
    ptts::level((const float*)dx, n, v, c, (float*)dy, stream_);
    PTTS_HIP(hipGetLastError());
    PTTS_HIP(hipMemcpyAsync(y, dy, sizeof(float) * n, hipMemcpyDeviceToHost, stream_));
    PTTS_HIP(hipStreamSynchronize(stream_));
  } catch (...) {
    (void)hipStreamSynchronize(stream_);
    (void)hipFree(dx), (void)hipFree(dy);
    throw;
  }
  (void)hipFree(dx), (void)hipFree(dy);
}

// ------------------------------------------------------------------ loudness stage
void Engine::loud_enable(bool on) {
  PTTS_REQUIRE(k_ == 0 && graphs_.empty(), "the loudness stage is chosen on an idle engine before its first step");
  PTTS_REQUIRE(!on || wire_, "the loudness stage needs a wire-enabled engine (ptts_wire_enable first)");
  PTTS_HIP(hipSetDevice(dev_));
  if (on && !loud_state_) {
    const size_t B = max_slots_;
    loud_coef(&loud_coef_);
    loud_state_ = (int*)dalloc(B * LOUD_STATE);
    loud_pend_ = dalloc(B * LOUD_SUB);
    loud_filt_ = (double*)dalloc(B * LOUD_FILT * 2);
    admit_loud_ = (int*)dalloc(B);
    h_loud_ = (int*)halloc(sizeof(int) * B);
  }
  if (on != loud_) {  // the blocks' head holds the records on a loudness-enabled engine only
    loud_ = on;
    wire_blocks_alloc();
  }
}

void Engine::fetch_loud(int calls_back, int B, double* energy, int* n_blocks) {
  PTTS_REQUIRE(loud_, "fetch_loud: the engine has no loudness stage (ptts_loud_enable)");
  PTTS_REQUIRE(B >= 1 && B <= max_slots_, "n_rows out of range");
  PTTS_REQUIRE(calls_back == 0 || calls_back == 1, "calls_back must be 0 or 1");
  PTTS_REQUIRE(energy != nullptr && n_blocks != nullptr, "null argument");
  // the same frame, rows and event as fetch_wire() of that call
  const int q = calls_back ? prev_hb_ : out_hb_;
  const int rows = calls_back ? prev_rows_ : out_rows_;
  const long long fk = calls_back ? prev_k_ : out_k_;
  if (pipeline_) PTTS_HIP(hipEventSynchronize(ev_back_[q - q % nfr_]));
  else sync();
  const int n = std::min(B, rows), f = q % nfr_;
  const unsigned char* blk = h_wireb_[nfr_ > 1 ? q / nfr_ : q];
  const LoudRecord* rec = (const LoudRecord*)(blk + wire_loud_off());
  for (int b = 0; b < B; ++b) {
    const size_t at = (size_t)b * nfr_ + f;
    int c = b < n ? rec[at].n_blocks : 0;  // (the stage writes every record of the pass's rows: 0 without a frame)
    if (c && !cancel_wins_.empty() && frame_cancelled(b, fk)) c = 0;  // as fetch_wire: nothing of that utterance
    if (c < 0 || c > LOUD_BLOCKS_MAX) throw Error(PTTS_ERR_STATE, "fetch_loud: corrupt block count");
    for (int i = 0; i < LOUD_BLOCKS_MAX; ++i) energy[(size_t)b * LOUD_BLOCKS_MAX + i] = i < c ? rec[at].e[i] : 0.0;
    n_blocks[b] = c;
  }
}

void Engine::loud_host(const float* x, int n, double* energy) {
  PTTS_REQUIRE(x && n >= 0 && (energy || n < LOUD_SUB), "null argument");
  if (n < LOUD_SUB) return;
  LoudCoef k;
  loud_coef(&k);
  sync();
  void *dx = nullptr, *de = nullptr;
  const size_t nb = (size_t)n / LOUD_SUB;
  try {
    PTTS_HIP(hipMalloc(&dx, sizeof(float) * n));
    PTTS_HIP(hipMalloc(&de, sizeof(double) * nb));
    PTTS_HIP(hipMemcpyAsync(dx, x, sizeof(float) * n, hipMemcpyHostToDevice, stream_));
    ptts::loud_blocks((const float*)dx, n, k, (double*)de, stream_);
    PTTS_HIP(hipGetLastError());
    PTTS_HIP(hipMemcpyAsync(energy, de, sizeof(double) * nb, hipMemcpyDeviceToHost, stream_));
    PTTS_HIP(hipStreamSynchronize(stream_));
  } catch (...) {
    (void)hipStreamSynchronize(stream_);
    (void)hipFree(dx), (void)hipFree(de);
    throw;
  }
  (void)hipFree(dx), (void)hipFree(de);
}

// ------------------------------------------------------------------ FLAC stage
void Engine::flac_enable(bool on) {
  PTTS_REQUIRE(k_ == 0 && graphs_.empty(), "the FLAC stage is chosen on an idle engine before its first step");
  PTTS_REQUIRE(!on || wire_, "the FLAC stage needs a wire-enabled engine (ptts_wire_enable first)");
  PTTS_HIP(hipSetDevice(dev_));
  if (on && !flac_first_) flac_first_ = (int*)dalloc((size_t)max_slots_ * nfr_);
  if (on != flac_) {  // the blocks' head holds the frame index on a FLAC-enabled engine only
    flac_ = on;
    wire_blocks_alloc();
  }
}

void Engine::fetch_flac_index(int calls_back, int B, int* index, int* n_frames) {
  PTTS_REQUIRE(flac_, "fetch_flac_index: the engine has no FLAC stage (ptts_flac_enable)");
  PTTS_REQUIRE(B >= 1 && B <= max_slots_, "n_rows out of range");
  PTTS_REQUIRE(calls_back == 0 || calls_back == 1, "calls_back must be 0 or 1");
  PTTS_REQUIRE(index != nullptr && n_frames != nullptr, "null argument");
  // the same frame, rows and event as fetch_wire() of that call
  const int q = calls_back ? prev_hb_ : out_hb_;
  const int rows = calls_back ? prev_rows_ : out_rows_;
  const long long fk = calls_back ? prev_k_ : out_k_;
  if (pipeline_) PTTS_HIP(hipEventSynchronize(ev_back_[q - q % nfr_]));
  else sync();
  const int n = std::min(B, rows), f = q % nfr_;
  const size_t slots = (size_t)max_slots_ * nfr_;
  const int* cnt = (const int*)h_wireb_[nfr_ > 1 ? q / nfr_ : q];
  memset(index, 0, sizeof(int) * 2 * FLAC_CHUNK_FRAMES * B);
  for (int b = 0; b < B; ++b) {
    const size_t at = (size_t)b * nfr_ + f;
    int c = b < n && cnt[at] ? cnt[slots + at] : 0;
    if (c && !cancel_wins_.empty() && frame_cancelled(b, fk)) c = 0;  // as fetch_wire: no byte of that utterance
    if (c < 0 || c > FLAC_CHUNK_FRAMES) throw Error(PTTS_ERR_STATE, "fetch_flac_index: corrupt frame count");
    long sum = 0;
    for (int i = 0; i < 2 * c; ++i) index[b * 2 * FLAC_CHUNK_FRAMES + i] = cnt[2 * slots + at * 2 * FLAC_CHUNK_FRAMES + i];
    for (int i = 0; i < c; ++i) sum += index[b * 2 * FLAC_CHUNK_FRAMES + 2 * i];
    if (c && sum != cnt[at]) throw Error(PTTS_ERR_STATE, "fetch_flac_index: the frame lengths do not sum to the chunk");
    n_frames[b] = c;
  }
}

long Engine::flac_bound(long n) { return n < 1 ? 0 : ptts::flac_bound(n); }

void Engine::flac_encode_host(const int16_t* x, int n, int rate, long long first, unsigned char* out, int* n_bytes,
                              int* index, int* n_frames) {
  PTTS_REQUIRE(x && out && n_bytes, "null argument");
  PTTS_REQUIRE((index == nullptr) == (n_frames == nullptr), "index and n_frames: both or neither");
  PTTS_REQUIRE(n >= 1 && n <= FLAC_CHUNK_SAMPLES, "flac_encode: n must be in [1, 11477]");
  const int ri = wire_rate_index(rate);
  PTTS_REQUIRE(ri >= 0, "sample_rate must be one of 8000, 16000, 24000, 44100, 48000");
  PTTS_REQUIRE(first >= 0 && first + n <= (1LL << 36), "first_sample outside the 36-bit sample number");
  const size_t cap = ((size_t)flac_bound(n) + 3) / 4 * 4;
  sync();
  void *dx = nullptr, *dy = nullptr, *dn = nullptr;
  int got[1 + 2 * FLAC_CHUNK_FRAMES] = {};  // the byte total, then the index
  const int nf = (n + FLAC_BLOCK - 1) / FLAC_BLOCK;
  try {
    PTTS_HIP(hipMalloc(&dx, sizeof(int16_t) * n));
    PTTS_HIP(hipMalloc(&dy, cap));
    PTTS_HIP(hipMalloc(&dn, sizeof(got)));
    PTTS_HIP(hipMemcpyAsync(dx, x, sizeof(int16_t) * n, hipMemcpyHostToDevice, stream_));
    ptts::flac_encode((const short*)dx, n, ri, first, (unsigned char*)dy, (int*)dn, index ? (int*)dn + 1 : nullptr, stream_);
    PTTS_HIP(hipGetLastError());
    PTTS_HIP(hipMemcpyAsync(got, dn, sizeof(int) * (index ? 1 + 2 * nf : 1), hipMemcpyDeviceToHost, stream_));
    PTTS_HIP(hipStreamSynchronize(stream_));
    if (got[0] < 1 || (size_t)got[0] > cap) throw Error(PTTS_ERR_STATE, "flac_encode: corrupt byte count");
    PTTS_HIP(hipMemcpy(out, dy, (size_t)got[0], hipMemcpyDeviceToHost));
  } catch (...) {
    (void)hipStreamSynchronize(stream_);
    (void)hipFree(dx), (void)hipFree(dy), (void)hipFree(dn);
    throw;
  }
  (void)hipFree(dx), (void)hipFree(dy), (void)hipFree(dn);
  *n_bytes = got[0];
  if (index) {
    memset(index, 0, sizeof(int) * 2 * FLAC_CHUNK_FRAMES);
    memcpy(index, got + 1, sizeof(int) * 2 * nf);
    *n_frames = nf;
  }
}

void Engine::mark_admission() {
  PTTS_HIP(hipEventRecord(ev_admit_, stream_));
  admit_pending_ = true;
  xh_dirty_ = true;  // lat_in_ (and, with a prefill, fbm_.x / fbm_.h) rewritten
}

// The reset of n staged slots (admit_slots_ / admit_st_ / admit_fpos_): the front-owned state and the
// codec state of bbm_ (conv histories, the overlap-add history, Mimi position), pending frame flags
ResetArgs Engine::reset_args(int n) const {
  ResetArgs r{};
  for (int i = 0; i < 8; ++i) {
    r.buf[i] = bbm_.hist[i];
    r.per_slot[i] = (long)hist_P_[i] * hist_C_[i];
  }
  r.buf[8] = bbm_.qprev;  // the overlap-add history
  r.per_slot[8] = MD;
  r.nb = 9;
  r.slots = admit_slots_;
  r.n = n;
  r.lat_in = lat_in_;
  r.bos = W(L_.bos);
  r.st_src = admit_st_;
  r.fpos_src = admit_fpos_;
  r.st = st_;
  r.fpos = fpos_;
  r.mpos = bbm_.mpos;
  for (int q = 0; q < NHB; ++q) r.flags[q] = flags_[q];
  return r;
}

// fbm_.x, fbm_.h rows of every slot from lat_in_ (the step's input projection + layer-0 norm1), on
// stream_ ahead of the next front part: after an admission, a voice prefill or anything else that
// used them as scratch or wrote lat_in_ (the step graphs keep them current themselves)
void Engine::refresh_xh() {
  input_ln(lat_in_, inw_t_, W(L_.fl[0].n1w), W(L_.fl[0].n1b), fbm_.x, fbm_.h, max_slots_, stream_);
  PTTS_HIP(hipGetLastError());
  xh_dirty_ = false;
}

// MimiModel::decode_from_latent (mimi.rs:143-157) with the denorm + quantize of tts_model.rs:
// 1033-1038 in front, on `slot`'s own streaming state, for n frames in sequence: the back part
// of the step plan run eagerly for rows [0, slot], only `slot` marked as carrying a frame.
// Every pending frame of the engine is dropped and the slot is reset first (use on an idle
// engine, as the reference's test_decoder_parity builds its own state). Optional outputs per
// frame: quant [512] (the 32 -> 512 quantizer output), up [16][512] (after the upsample
// convtr), tr [16][512] (after the decoder transformer), time-major.
void Engine::decode_latents(int slot, const float* lat, int n, float* pcm, float* quant, float* up, float* tr) {
  PTTS_REQUIRE(ready_, "engine weights not finalized");
  PTTS_REQUIRE(slot >= 0 && slot < max_slots_, "slot out of range");
  PTTS_REQUIRE(lat != nullptr && n >= 1, "no latents");
  sync();
  for (int q = 0; q < NHB; ++q) PTTS_HIP(hipMemsetAsync(flags_[q], 0, sizeof(FrameFlags) * max_slots_, stream_));
  {
    SlotState s{};
    s.eos_step = -1;
    *h_slots_ = slot;
    *h_st_ = s;
    *h_fp_ = 0;
    PTTS_HIP(hipMemcpyAsync(admit_slots_, h_slots_, sizeof(int), hipMemcpyHostToDevice, stream_));
    PTTS_HIP(hipMemcpyAsync(admit_st_, h_st_, sizeof(SlotState), hipMemcpyHostToDevice, stream_));
    PTTS_HIP(hipMemcpyAsync(admit_fpos_, h_fp_, sizeof(int), hipMemcpyHostToDevice, stream_));
    slot_reset(reset_args(1), stream_);
    PTTS_HIP(hipGetLastError());
  }
  const FrameFlags on{1, 0}, off{0, 0};
  auto rows16 = [&](float* dst, const float* src) {  // the slot's 16 Mimi rows [16][512]
    PTTS_HIP(hipMemcpyAsync(dst, src + (size_t)slot * UP * MD, sizeof(float) * UP * MD, hipMemcpyDeviceToHost,
                            stream_));
  };
  for (int i = 0; i < n; ++i) {
    const int par = i & 1;  // the frame's hand-off buffer
    PTTS_HIP(hipMemcpyAsync(lat_out_[par] + (size_t)slot * LDIM, lat + (size_t)i * LDIM, sizeof(float) * LDIM,
                            hipMemcpyHostToDevice, stream_));
    PTTS_HIP(hipMemcpyAsync(flags_[par] + slot, &on, sizeof on, hipMemcpyHostToDevice, stream_));
    BackPass pass;  // one frame from buffer par into pcm_[par]; the seam decodes to f32 only: no wire block
    pass.lat[0] = lat_out_[par];
    pass.flags[0] = flags_[par];
    pass.pcm = pcm_[par];
    std::vector<Op> ops;
    build_back(ops, slot + 1, bbm_, pass);
    size_t j = 0;
    for (; j < ops.size(); ++j) {
      if (ops[j].name == "seanet.conv0" && tr) rows16(tr + (size_t)i * UP * MD, bbm_.mx);
      ops[j].fn(stream_);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) throw Error(PTTS_ERR_HIP, "launch of " + ops[j].name + " failed: " + hipGetErrorString(e));
      if (j == 0 && up) rows16(up + (size_t)i * UP * MD, bbm_.mx);
    }
    if (pcm)
      PTTS_HIP(hipMemcpyAsync(pcm + (size_t)i * FRAME, pass.pcm + (size_t)slot * FRAME, sizeof(float) * FRAME,
                              hipMemcpyDeviceToHost, stream_));
    if (quant)
      PTTS_HIP(hipMemcpyAsync(quant + (size_t)i * MD, bbm_.qcur + (size_t)slot * NFR_MAX * MD,
                              sizeof(float) * MD, hipMemcpyDeviceToHost, stream_));
    PTTS_HIP(hipMemcpyAsync(flags_[par] + slot, &off, sizeof off, hipMemcpyHostToDevice, stream_));
    PTTS_HIP(hipStreamSynchronize(stream_));
  }
  mark_admission();
  drained_[slot] = 1;
  codec_ok_[slot] = 0;  // not an utterance's state
  pv_forget(slot);
}

void Engine::slot_close(int slot) {
  PTTS_REQUIRE(slot >= 0 && slot < max_slots_, "slot out of range");
  sync();
  act_slots_.erase(std::remove(act_slots_.begin(), act_slots_.end(), slot), act_slots_.end());
  SlotState s{};
  s.eos_step = -1;
  memcpy(h_st_, &s, sizeof s);  // pinned staging (free: sync() above)
  PTTS_HIP(hipMemcpyAsync(st_ + slot, h_st_, sizeof s, hipMemcpyHostToDevice, stream_));
  for (int q = 0; q < NHB; ++q)  // drop a pending frame of the slot
    PTTS_HIP(hipMemsetAsync(flags_[q] + slot, 0, sizeof(FrameFlags), stream_));
  if (align_ && slot_align_[slot]) {
    PTTS_HIP(hipMemsetAsync(align_tab_ + slot, 0, sizeof(AlignEntry), stream_));
    slot_align_[slot] = 0;
  }
  if (share_voice_ && slot_voice_[slot]) {  // the closed row (still stepped, discarded) reads its own rows
    h_vpre_[slot] = nullptr;
    h_vlen_[slot] = 0;
    PTTS_HIP(hipMemcpyAsync(vpre_ + slot, h_vpre_ + slot, sizeof(float*), hipMemcpyHostToDevice, stream_));
    PTTS_HIP(hipMemcpyAsync(vlen_ + slot, h_vlen_ + slot, sizeof(int), hipMemcpyHostToDevice, stream_));
  }
  mark_admission();
  PTTS_HIP(hipStreamSynchronize(stream_));
  drained_[slot] = 1;
  codec_ok_[slot] = 0;
  cancelled_[slot] = 0;
  pv_forget(slot);
  voice_release(slot, true);
}

// Stream-ordered cancel: nothing here waits for the GPU. The idle state lands on the front stream
// behind the front parts already issued (SlotState is front-owned: no back part reads it), from a
// pinned constant, so no staging has to come free first. The rows' frames still in flight are
// decoded as queued (other rows' passes are untouched) and masked on the host by their call
// index. drained_ stays 0: a queued back pass may still write the slot's histories, so the slot's
// next admission takes the ev_be_tail_ wait; the voice reference is kept until then as well (the
// idle row is still stepped and reads its prefix).
void Engine::slots_cancel(int n, const int* slots) {
  PTTS_REQUIRE(ready_, "engine weights not finalized");
  PTTS_REQUIRE(n >= 0 && n <= max_slots_ && (n == 0 || slots != nullptr), "number of slots out of range");
  std::vector<char> seen(max_slots_, 0);
  for (int i = 0; i < n; ++i) {
    PTTS_REQUIRE(slots[i] >= 0 && slots[i] < max_slots_, "slot out of range");
    PTTS_REQUIRE(!seen[slots[i]], "slot cancelled twice in one call");
    seen[slots[i]] = 1;
  }
  PTTS_HIP(hipSetDevice(dev_));
  for (int i = 0; i < n; ++i) {
    const int slot = slots[i];
    if (drained_[slot] || cancelled_[slot]) continue;  // idle, finished or never admitted: nothing to stop
    PTTS_HIP(hipMemcpyAsync(st_ + slot, h_idle_, sizeof(SlotState), hipMemcpyHostToDevice, stream_));
    if (align_ && slot_align_[slot]) {  // out of the align stage, in the same stream order (no staging)
      PTTS_HIP(hipMemsetAsync(align_tab_ + slot, 0, sizeof(AlignEntry), stream_));
      slot_align_[slot] = 0;
    }
    // admitted inside a multi-frame pass and not started yet: it never starts
    act_slots_.erase(std::remove(act_slots_.begin(), act_slots_.end(), slot), act_slots_.end());
    cancelled_[slot] = 1;
    codec_ok_[slot] = 0;
    slot_lsd_[slot] = 0;  // lsd_run_for: the row counts no more
    if (k_ > admit_call_[slot]) cancel_wins_.push_back({slot, admit_call_[slot], k_});
    pv_forget(slot);
  }
}

void Engine::voice_release(int slot, bool drained) {
  const ptts_voice* v = slot_voice_[slot];
  if (!v) return;
  slot_voice_[slot] = nullptr;
  bool free_now = false;
  {
    std::lock_guard<std::mutex> lk(voice_mu());
    free_now = --v->refs == 0 && v->dead;
  }
  if (!free_now) return;
  if (!drained) PTTS_HIP(hipStreamSynchronize(stream_));  // queued steps may still read it
  free_voice(const_cast<ptts_voice*>(v));
}

void voice_destroy(ptts_voice* v) {
  if (!v) return;
  {
    std::lock_guard<std::mutex> lk(voice_mu());
    if (v->refs > 0) {  // slots still read it: the last to let go frees it
      v->dead = true;
      return;
    }
  }
  free_voice(v);  // waits for a pending job of the voice first
}

void Engine::set_latent(int slot, const float* lat) {
  PTTS_REQUIRE(slot >= 0 && slot < max_slots_ && lat != nullptr, "bad slot / latent");
  sync();
  PTTS_HIP(hipMemcpyAsync(lat_in_ + (size_t)slot * LDIM, lat, sizeof(float) * LDIM, hipMemcpyHostToDevice, stream_));
  mark_admission();
  PTTS_HIP(hipStreamSynchronize(stream_));
}

// ---- first-frame previews --------------------------------------------------------------------
// The pipelined engine returns a row's frame k frame_lag() calls after the call that computed its
// latent (2 n - 1 with n-frame passes): the back passes decode every row's frames together, so the
// first frame of a new utterance waits for a pass over frames of all rows. A preview decodes the
// first frame of each newly started row right after its front part, alone: a single-frame back
// pass over those rows (their latents gathered from the call's hand-off buffer into a compact
// batch of P = 1, 2, 4 or 8 rows) on its own high-priority stream, from the fresh Mimi decoder
// state every utterance starts from (tts_model.rs:941 init_states; zero conv and overlap-add
// histories, empty attention ring). That is exactly the state the row's regular pass decodes its
// frame 0 from, so the preview is that frame up to float rounding of the other tile shapes; the
// regular pass still decodes it (it advances the row's own state), and the caller delivers the
// first of the two to arrive (serve.py BatchScheduler).
void Engine::preview_enable(int max_rows) {
  static_assert(PV_MAX <= GATHER_MAX, "preview rows travel in the gather's arguments");
  PTTS_REQUIRE(max_rows >= 0 && max_rows <= PV_MAX, "preview rows must be in [0, 8]");
  PTTS_REQUIRE(max_rows == 0 || pipeline_, "first-frame previews: pipelined engines only");
  PTTS_HIP(hipSetDevice(dev_));
  if (max_rows > 0 && !stream_pv_) {
    const size_t P = PV_MAX;
    pv_ = back_alloc(PV_MAX, 1);
    pv_lat_ = dalloc(P * LDIM);
    pv_flags_ = (FrameFlags*)dalloc(P * 2);
    pv_pcm_ = dalloc(P * FRAME);
    for (PvEntry& q : pv_q_) {
      PTTS_HIP(hipEventCreateWithFlags(&q.ev, hipEventDisableTiming));
      q.h_pcm = (float*)halloc(sizeof(float) * P * FRAME);
    }
    for (int q = 0; q < NHB; ++q) PTTS_HIP(hipEventCreateWithFlags(&ev_pv_read_[q], hipEventDisableTiming));
    PTTS_HIP(hipEventCreateWithFlags(&ev_pv_front_, hipEventDisableTiming));
    int lo = 0, hi = 0;  // the preview is the one latency-bound part: the highest stream priority
    PTTS_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
    PTTS_HIP(hipStreamCreateWithPriority(&stream_pv_, hipStreamNonBlocking, hi));
  }
  pv_max_ = max_rows;
  if (!max_rows) pv_pending_.clear();
  for (int P = 1; P < 2 * max_rows; P *= 2) pv_graph(P);  // instantiated now, not at a first chunk
}

void Engine::pv_forget(int slot) {
  pv_pending_.erase(std::remove_if(pv_pending_.begin(), pv_pending_.end(),
                                   [slot](const std::pair<int, long long>& p) { return p.first == slot; }),
                    pv_pending_.end());
  for (int i = 0; i < pv_count_; ++i) {
    PvEntry& e = pv_q_[(pv_head_ + i) % PV_Q];
    for (int j = 0; j < e.n; ++j)
      if (e.slots[j] == slot) e.slots[j] = -1;
  }
}

// the preview pass over P compact rows (built once per P, captured on stream_pv_)
hipGraphExec_t Engine::pv_graph(int P) {
  auto it = pv_graphs_.find(P);
  if (it != pv_graphs_.end()) return it->second;
  // One frame of the gathered batch over the previews' own workspace, f32 at 24 kHz only (no wire
  // block). The preview state must stay the fresh one (zero conv and overlap-add histories, Mimi
  // position 0): the pass's closing commit, the only op that writes it, is left out, so the buffers
  // keep the zeros dalloc gave them and no reset runs per preview. (The attention ring is rewritten
  // at positions 0..15 by each preview before it reads them. The small-row path has no fused final
  // conv, whose tile-boundary shares the commit would otherwise add.)
  PTTS_REQUIRE(P < 16, "preview pass: the small-row path only");
  BackPass pass;
  pass.lat[0] = pv_lat_;
  pass.flags[0] = pv_flags_;
  pass.pcm = pv_pcm_;
  pass.commit = false;
  std::vector<Op> ops;
  build_back(ops, P, pv_, pass);
  hipGraph_t g = nullptr;
  PTTS_HIP(hipStreamBeginCapture(stream_pv_, hipStreamCaptureModeThreadLocal));
  try {
    set_wg_cap(0);
    set_back_hi(1);
    for (const Op& op : ops) op.fn(stream_pv_);
  } catch (...) {
    (void)hipStreamEndCapture(stream_pv_, &g);
    throw;
  }
  PTTS_HIP(hipStreamEndCapture(stream_pv_, &g));
  hipGraphExec_t ge = nullptr;
  PTTS_HIP(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
  pv_graph_defs_[P] = g;
  pv_graphs_[P] = ge;
  return ge;
}

// After the front part of call k_ (buffer hb, rows [0, B)) is queued on stream_: the previews of
// the rows whose first front part that is (rows past B, or past pv_max_ rows, or with the FIFO
// full, take the regular path only)
void Engine::launch_previews(int B, int hb) {
  if (pv_max_ <= 0 || pv_pending_.empty()) return;
  std::vector<int> rows;
  std::vector<std::pair<int, long long>> keep;
  for (const auto& p : pv_pending_) {
    if (p.second > k_) keep.push_back(p);
    else if (p.second == k_ && p.first < B && (int)rows.size() < pv_max_) rows.push_back(p.first);
  }
  pv_pending_.swap(keep);
  if (rows.empty() || pv_count_ == PV_Q) return;
  const int n = (int)rows.size();
  int P = 1;
  while (P < n) P *= 2;
  hipGraphExec_t graph = pv_graph(P);
  PvEntry& e = pv_q_[(pv_head_ + pv_count_) % PV_Q];  // free: fetched (its copies done) or never used
  e.n = n;
  for (int i = 0; i < n; ++i) e.slots[i] = rows[i];
  PTTS_HIP(hipEventRecord(ev_pv_front_, stream_));
  PTTS_HIP(hipStreamWaitEvent(stream_pv_, ev_pv_front_, 0));
  gather_preview(lat_out_[hb], flags_[hb], rows.data(), n, P, pv_lat_, pv_flags_, stream_pv_);
  PTTS_HIP(hipGetLastError());
  PTTS_HIP(hipEventRecord(ev_pv_read_[hb], stream_pv_));  // front(k + nhb_) rewrites buffer hb
  pv_read_pending_[hb] = true;
  PTTS_HIP(hipGraphLaunch(graph, stream_pv_));
  PTTS_HIP(hipMemcpyAsync(e.h_pcm, pv_pcm_, sizeof(float) * n * FRAME, hipMemcpyDeviceToHost, stream_pv_));
  PTTS_HIP(hipEventRecord(e.ev, stream_pv_));
  ++pv_count_;
}

// Completed previews in launch order, whole previews only, at most max_n frames: slots[i] and
// pcm[i * 1920 ..]. wait: block until the launched previews complete (as many as fit).
int Engine::preview_fetch(int wait, int max_n, int* slots, float* pcm) {
  PTTS_REQUIRE(max_n >= 0 && (max_n == 0 || (slots && pcm)), "preview_fetch: null outputs");
  int got = 0;
  while (pv_count_ > 0) {
    PvEntry& e = pv_q_[pv_head_];
    int live = 0;
    for (int j = 0; j < e.n; ++j) live += e.slots[j] >= 0;
    if (got + live > max_n) break;
    if (wait) {
      PTTS_HIP(hipEventSynchronize(e.ev));
    } else {
      const hipError_t r = hipEventQuery(e.ev);
      if (r == hipErrorNotReady) {
        (void)hipGetLastError();  // not an error: clear it for the next PTTS_HIP(hipGetLastError())
        break;
      }
      PTTS_HIP(r);
    }
    for (int j = 0; j < e.n; ++j)
      if (e.slots[j] >= 0) {
        slots[got] = e.slots[j];
        memcpy(pcm + (size_t)got * FRAME, e.h_pcm + (size_t)j * FRAME, sizeof(float) * FRAME);
        ++got;
      }
    pv_head_ = (pv_head_ + 1) % PV_Q;
    --pv_count_;
  }
  return got;
}

}  // namespace ptts
