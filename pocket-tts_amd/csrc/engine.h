// Batched Pocket TTS engine: owns device weights, per-slot streaming state and the step plan.
#pragma once
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "common.h"
#include "kernels.h"
#include "weights.h"

// Immutable voice prefix (the reference's ModelState after the prompt prefill,
// tts_model.rs:490-501 / 504-560): FlowLM KV for F conditioning positions.
// Slots read the prefix from this copy (shared voice prefixes, KvStore::pre): `refs` counts the
// slots that do, and ptts_voice_destroy on a referenced voice only marks it `dead`; the last
// slot to let go of it frees it (ptts::voice_destroy, Engine::voice_release).
struct ptts_voice {
  int F = 0;
  float* kv = nullptr;      // device [NL][2][NH][F][64]
  std::vector<float> cond;  // conditioning rows [F][1024] (kept for PCM voices)
  const void* owner = nullptr;
  mutable int refs = 0;
  mutable bool dead = false;
  // voice jobs (Engine::voice_job_*): the event recorded on the voice stream behind the job (null:
  // made synchronously), the pinned host copy of the conditioning the job's last copy fills (PCM
  // jobs), and whether the front stream has already been ordered behind the event
  hipEvent_t ev = nullptr;
  float* h_cond = nullptr;
  mutable bool ordered = false;
};

namespace ptts {

struct VoicePlan;  // engine.cpp: what the host works out about a clip before a clone is enqueued

// ptts_voice_destroy: frees the voice now, or (while slots still read its prefix) marks it for
// the last of them to free
void voice_destroy(ptts_voice* v);

struct Op {
  std::string name;
  std::function<void(hipStream_t)> fn;
  double flops = 0, bytes = 0;  // algorithmic cost of one launch (GEMM/conv ops)
  // state an isolated replay of `fn` needs first (time_op), which the step's previous ops provide
  std::function<void(hipStream_t)> prep = nullptr;
};

class Engine {
 public:
  explicit Engine(const ptts_engine_config& cfg);
  ~Engine();
  Engine(const Engine&) = delete;
  Engine& operator=(const Engine&) = delete;

  void finalize();
  void load_blob(const float* host, size_t n_bytes);
  float* blob() { return blob_; }
  int max_slots() const { return max_slots_; }
  bool pipelined() const { return pipeline_; }
  // calls by which a frame trails its FlowLM step (ptts_frame_lag) and the latest admission's
  // start delay
  // (a pass over nfr frames: 2 nfr - 1 calls; single frames: 1)
  int frame_lag() const { return !pipeline_ ? 0 : 2 * nfr_ - 1; }
  int admit_delay() const { return admit_delay_; }

  // One clone (voice_clone), called synchronously: drains the pipeline, returns the finished voice
  ptts_voice* voice_from_prompt(const float* prompt, int F);
  ptts_voice* voice_from_pcm(const float* pcm, int n) { return voice_from_audio(pcm, n, PTTS_SAMPLE_RATE, 0); }
  // resampler: PTTS_RESAMPLE_POLY (resample_poly rule) or PTTS_RESAMPLE_RUBATO_SEPTIC (the Rust driver's)
  ptts_voice* voice_from_audio(const float* x, int n, int sample_rate, int chunk_frames,
                               int resampler = PTTS_RESAMPLE_POLY);
  void resample_host(const float* x, int n, int sr_from, int sr_to, float* y, int resampler = PTTS_RESAMPLE_POLY);
  // or as a job on the engine's voice stream: returns at once, the voice is admissible immediately
  // (slots_open orders the front stream behind the job's event). sample_format: PTTS_SAMPLES_F32 / _S16
  ptts_voice* voice_job_audio(const void* samples, int n, int sample_format, int sample_rate, int chunk_frames,
                              int resampler);
  ptts_voice* voice_job_prompt(const float* prompt, int F);
  void voice_jobs_reserve(int max_frames);
  // lsd_steps: the utterance's own Euler step count in [1, cap], or 0 (nullptr: every entry 0) for
  // the engine's default, the cap (cfg.lsd_decode_steps)
  void slot_open(int slot, const ptts_voice* v, const int32_t* ids, int n, const ptts_gen_params& p,
                 int lsd_steps = 0);
  // opts: one entry per row, this library's own struct whole (its fields: pocket_tts.h; `size` is
  // not read here), or nullptr for the defaults in every row. A prefix is read before the call returns
  void slots_open(int n, const int* slots, const ptts_voice* const* voices, const int32_t* ids, const int* n_ids,
                  const ptts_gen_params* params, const ptts_slot_opts* opts);
  int lsd_cap() const { return lsd_; }
  int lsd_last_run() const { return lsd_last_run_; }  // Euler steps of the latest front part (0: none yet)
  void slot_close(int slot);
  // Stop the utterances of n distinct slots without draining the pipeline (ptts_slots_cancel;
  // DESIGN.md section 18): stream-ordered like slots_open, no host wait. Frames of the cancelled
  // utterances still in flight are masked in the fetch path.
  void slots_cancel(int n, const int* slots);
  void set_latent(int slot, const float* lat);
  void decode_latents(int slot, const float* lat, int n, float* pcm, float* quant, float* up, float* tr);

  void step_async(int B);
  // a pipelined call that starts no frame (ptts_flush_async): only the back parts of frames
  // already computed advance, so a caller whose rows have all finished drains the pipeline
  // without running front parts whose frames would be discarded
  void flush_async(int B);
  void sync();
  // the frame of the call calls_back (0 or 1) calls before the latest
  void fetch(int B, float* pcm, uint8_t* valid, uint8_t* last, float* eos, float* lat, int calls_back = 0);
  // fetch() of that call would not block (its frame's back pass has completed)
  bool fetch_ready(int calls_back);
  // the front part of the call calls_back (0..3) calls before the latest has completed (wait:
  // block until it has); true for calls before the first
  bool front_done(int calls_back, bool wait);

  // First-frame previews (ptts_preview_enable / ptts_preview_fetch): the first frame of up to
  // max_rows rows that start in one call is also decoded right after that call's front part, by a
  // single-frame back pass over those rows alone on a third stream, from a fresh Mimi state (the
  // state every utterance starts from), so a new stream's first chunk does not wait the
  // pipeline's frame lag. The rows' regular frame 0 is still decoded (it advances their state);
  // the caller delivers whichever arrives first.
  void preview_enable(int max_rows);
  int preview_fetch(int wait, int max_n, int* slots, float* pcm);

  // Wire stage (ptts_wire_enable / ptts_fetch_wire): with it on, every back
  // pass ends in one more launch that turns the f32 PCM of the rows that asked for a format into
  // their wire bytes (kernels.h wire_stage), and one more copy carries them to pinned host memory.
  // Valid before the engine's first call only (the back graphs are captured with or without it).
  void wire_enable(bool on);
  bool wire() const { return wire_; }
  // the wire chunks of the frame fetch(.., calls_back) returns: n_bytes[b] bytes at out + b * row_stride
  void fetch_wire(int calls_back, int B, unsigned char* out, size_t row_stride, int* n_bytes);
  // the seam alone: whole-signal f32 at 24 kHz -> wire bytes (wire_len of them)
  static long wire_len(long n_samples, int rate, int enc);  // -1: unknown rate or encoding
  void wire_encode_host(const float* pcm, int n, int rate, int enc, unsigned char* out);
  // Tempo stage (ptts_tempo_enable): rows admitted with a speed have their PCM
  // time-scaled (kernels.h tempo_stage) ahead of the wire stage; chunks grow to wire_chunk_max()
  void tempo_enable(bool on);
  bool tempo() const { return tempo_; }
  int wire_chunk_max() const { return level_ ? WIRE_CHUNK_MAX_LEVEL : tempo_ ? WIRE_CHUNK_MAX_TEMPO : WIRE_CHUNK_MAX; }
  // the seam alone: whole-signal f32 at 24 kHz -> tempo_len(n, sp) samples
  void tempo_host(const float* pcm, int n, int sp, float* out);
  // Pitch stage (ptts_pitch_enable): rows admitted with pitch_cents have their
  // (time-scaled) PCM resampled by a fractional ratio (kernels.h pitch_stage) between the tempo and
  // the wire stage; needs the tempo stage, keeps its chunk slots
  void pitch_enable(bool on);
  bool pitch() const { return pitch_; }
  // the seam alone: whole-signal f32 -> pitch_len(n, step) samples
  void pitch_host(const float* x, int n, unsigned step, float* y);
  // Level stage (ptts_level_enable): rows admitted with a gain or `limit` have
  // their (time-scaled, pitch-shifted) PCM scaled and peak-limited to the engine's ceiling (kernels.h
  // level_stage) ahead of the wire stage; needs the wire stage only; chunk slots grow to
  // WIRE_CHUNK_MAX_LEVEL
  void level_enable(bool on, int ceiling_cdb);
  bool level() const { return level_; }
  long level_min_chunk() const;  // the smallest non-last chunk of a level row over the engine's stages (samples)
  // the seam alone: whole-signal f32 -> n samples
  void level_host(const float* x, int n, int gain_cdb, int ceiling_cdb, float* y);
  // Loudness stage (ptts_loud_enable): rows admitted with ptts_slot_opts.loud
  // have the signal the wire stage reads metered (kernels.h loud_stage); needs the wire stage only.
  // The records ride in the pass blocks' head; no chunk slot changes size
  void loud_enable(bool on);
  bool loud() const { return loud_; }
  void fetch_loud(int calls_back, int B, double* energy, int* n_blocks);
  // the seam alone: whole-signal f32 -> n / LOUD_SUB sub-block energies
  void loud_host(const float* x, int n, double* energy);
  // FLAC stage (ptts_flac_enable): rows admitted with PTTS_WIRE_FLAC have their
  // 16-bit chunks encoded as FLAC frames (kernels.h flac_stage) behind the wire stage
  void flac_enable(bool on);
  bool flac() const { return flac_; }
  static long flac_bound(long n);  // bytes of an n-sample chunk's frames, at most (0: n < 1)
  // the seam alone: the stage's chunk encoder on n 16-bit samples at `rate`; index [3][2] and n_frames
  // (both or neither) receive each frame's byte length and block size, and the frame count
  void flac_encode_host(const int16_t* x, int n, int rate, long long first, unsigned char* out, int* n_bytes,
                        int* index, int* n_frames);
  // the frame index of the chunks fetch_wire(calls_back, ..) returns (section 21.5): index [B][3][2]
  // (byte length, block size; zeros behind n_frames[b]); the same event, no bookkeeping of its own
  void fetch_flac_index(int calls_back, int B, int* index, int* n_frames);

  // Align stage (ptts_align_enable / ptts_fetch_align): with it on, the front
  // part has one more launch behind layer `layer`'s step attention, which writes the text-attention
  // row (mean over the heads of head_mask) of every row admitted with align = 1 into the frame's
  // hand-off buffer; the rows travel with the frame. Valid before the engine's first call only.
  void align_enable(bool on, int layer, unsigned head_mask);
  bool align() const { return align_; }
  // the alignment rows of the frame fetch(.., calls_back) returns: n_tokens[b] floats at out + b * row_stride
  void fetch_align(int calls_back, int B, float* out, size_t row_stride, int* n_tokens);
  // the seam alone: align_step on host operands (ptts_test_align)
  void test_align(int M, int nh, int cap, int S, const float* qkv, const float* kvh, const float* pre,
                  const int* pre_len, const int* pos, const int* tab, unsigned head_mask, float* out);

  double time_op(int B, const std::string& name, int reps);
  // GEMM-core test hook (ptts_test_gemm): Y = X W^T on tile `layout` (host buffers)
  void test_gemm(int layout, int M, int N, int K, int splits, int tail_S, const float* X, const float* Wt, float* Y);
  // Attention-path test hook (ptts_test_attention): the product launchers on host operands
  void test_attention(int kind, int M, int nh, int cap, int window, int n_slots, int S, const float* qkv, float* kvh,
                      const float* pre, const int* pre_len, int slot0, int rps, int p0, const int* pos, const int* tab,
                      const int* ptab, int mpad, float* Qh, float* Oh);
  // Row-reduce test hook (ptts_test_row_reduce): the product launcher on host operands
  void test_row_reduce(int M, int N, int S, int act, int ln, float eps, int front, const float* P, const float* bias,
                       const float* gate, const float* R, const float* ln_w, const float* ln_b, const float* mscale,
                       const float* mshift, float* Y, float* H, float* Hfrag);
  void overlap_probe(int B, int reps, double* us);
  std::vector<std::string> plan_names(int B);
  int int8_matrices() const { return (int)q8map_.size(); }
  int fp8_matrices() const { return (int)f8map_.size(); }

 private:
  float* dalloc(size_t n);      // device memory (zeroed) and pinned host memory whose lifetime is the
  void* halloc(size_t bytes);   // engine's: tracked in allocs_ / hallocs_, freed by the destructor
  const float* W(size_t off) const { return blob_ + off; }
  void upload_weights(TensorSource* src);
  void derive_int8();
  void derive_fp8();
  // Every pass is built over an explicit workspace. FlowLM side, what flow_layers / linear_split
  // write: the engine's own (fbm_: step and admission graphs) or a voice clone's (VoiceWs). kv is layer
  // 0's store (fbm_'s carries the shared voice prefixes); layer l's base is kv.base + l * kv_layer.
  struct FlowBufs {
    float *x = nullptr, *h = nullptr, *q = nullptr, *o = nullptr, *u = nullptr, *partial = nullptr;
    size_t pcap = 0;
    float* tslab = nullptr;
    long tail_cap = 0;
    int* tickets = nullptr;
    KvStore kv{};  // [max_slots][NL][2][NH][max_ctx][64]
    long kv_layer = 0;
  };
  FlowBufs fbm_{};
  // Mimi / SEANet side: the workspace and per-row codec state build_back reads and writes, the
  // engine's own (bbm_: max_slots rows, back_frames frames per pass) or the previews' (pv_)
  struct BackBufs {
    float *ring = nullptr, *qprev = nullptr, *qcur = nullptr, *mx = nullptr, *mh = nullptr, *mq = nullptr,
          *mo = nullptr, *mqkv = nullptr, *mu = nullptr, *a0 = nullptr, *mpartial = nullptr, *fin_side = nullptr;
    float *cb[3] = {}, *cv[3] = {}, *ca[3] = {}, *ce[3] = {}, *hist[8] = {};
    int* mpos = nullptr;
    size_t mpcap = 0;  // floats of mpartial, the back part's own split-K slabs
  };
  BackBufs bbm_{};
  BackBufs back_alloc(int rows, int nfr);
  // The frames one back pass decodes and where its output goes
  struct BackPass {
    int nfr = 1;
    const float* lat[NFR_MAX] = {};  // per frame f < nfr: latents [B][32] and frame flags [B]
    const FrameFlags* flags[NFR_MAX] = {};
    float* pcm = nullptr;  // frame f of row b at pcm + b * pcm_ld + f * FRAME
    long pcm_ld = FRAME;
    unsigned char* wire = nullptr;  // the pass's wire block; null: no wire / tempo ops
    bool commit = true;             // the pass ends in the commit of the rows' codec state
  };
  BackPass step_pass(int hb, int nfr) const;  // the engine's own pass over hand-off buffers hb .. hb + nfr - 1
  ResetArgs reset_args(int n) const;  // the slot_reset of n staged admissions
  void prefill_rows(std::vector<Op>& ops, int slot, int T, int p0, const FlowBufs& fb);
  void run_ops(const std::vector<Op>& ops);
  void run_ops_on(const std::vector<Op>& ops, hipStream_t s);
  std::vector<Op> build_step(int B);
  // hb: front -> back hand-off buffer (frame index mod NHB); qp: the back part's frame index mod 2
  void build_front(std::vector<Op>& ops, int B, int hb, int lsd_run);
  void build_back(std::vector<Op>& ops, int B, const BackBufs& bb, const BackPass& pass);
  // multi-frame passes: a pass whose later calls were all flushes decodes only the frames its
  // calls started (nfr in part_graph's key)
  // (front parts: lsd_run, the Euler steps the graph runs, is part of the key too)
  hipGraphExec_t part_graph(int part, int B, int hb, int qp, int nfr, int lsd_run = 0);
  void wait_unless_done(hipStream_t s, hipEvent_t e);
  void copy_out(int B, int hb, hipStream_t s);
  void push_rr(std::vector<Op>& ops, const std::string& name, const RowReduceArgs& r);
  // align_out: the step's alignment rows (build_front of an align-enabled engine), or nullptr
  void flow_layers(std::vector<Op>& ops, int M, RowMap map, bool step, bool out_norm, const std::string& tag,
                   const FlowBufs& fb, float* align_out = nullptr);
  void linear_split(std::vector<Op>& ops, const std::string& name, const float* X, long ldx, int M, const float* Wt,
                    int N, int K, int* S_out, const FlowBufs& fb);
  void conv_op(std::vector<Op>& ops, const std::string& name, const float* X, int B, int T_in, int cin, const float* H,
               int P, int stride, int elu, const float* Wt, int cout, int ktaps, int phases, const float* bias,
               const float* R, float* Y, int T_out, int tstride, int layout = TILE_KSPLIT_4W, int elu_out = 0,
               float* Y2 = nullptr, int ksplit = 1, float* slabs = nullptr, size_t slab_cap = 0);
  void dense_op(std::vector<Op>& ops, const std::string& name, const float* X, int M, const float* Wt, int N, int K,
                const float* bias, int act, const float* rscale, const float* R, float* Y,
                int layout = TILE_KSPLIT_4W);
  void encoder_transformer(std::vector<Op>& ops, float* x, int T, float* h, float* qkv, float* q, float* o, float* u,
                           float* ring);

  // configuration
  // lsd_: cfg.lsd_decode_steps, the cap on (and default of) the per-row Euler step counts
  static constexpr int LSD_MAX = 64;
  int dev_ = 0, max_slots_ = 0, max_ctx_ = 0, lsd_ = 1;
  std::vector<int> slot_lsd_;  // per slot: the count of its current utterance (0: never admitted)
  int lsd_last_run_ = 0;
  int lsd_run_for(int B) const;
  int wq_ = 0;  // weight_quant mode (QuantMode)
  // int8 code matrices of the quantized FlowLM step GEMMs: f32 weight pointer -> (codes, row scales)
  std::map<const float*, std::pair<const int8_t*, const float*>> q8map_;
  int fp8_ = 0;  // ptts_engine_config.fp8_gemm
  // e4m3 code matrices of the large FlowLM step GEMMs: f32 weight pointer -> (codes, row scales)
  std::map<const float*, std::pair<const uint8_t*, const float*>> f8map_;
  // fragment-packed copies of the f32 FlowLM step matrices for gemv_splitk: weight -> (copy, shape)
  struct Gemv {
    const float* packed;
    GemvShape g;
    int bit;  // PTTS_GEMV mask bit of the matrix
    const uint32_t* q8;   // weight_quant engines: the int8 codes in pack_q8 order, or nullptr
    const float* scale;   // their row scales
  };
  // int8 codes of a quantized matrix in the fragment order `pack` gives its f32 values (pack_q8)
  const uint32_t* pack_codes(const float* W, int N, int K, int nj, const std::function<void(const float*, float*)>& pack);
  // fused feed-forward of weight_quant engines: linear2 weight -> ((linear1 codes, scales), (linear2 codes, scales))
  std::map<const float*, std::pair<std::pair<const uint32_t*, const float*>, std::pair<const uint32_t*, const float*>>>
      ffn8map_;
  std::map<const float*, Gemv> gvmap_;
  // whole-K copies of the FlowLM linear1 matrices for gemv_fk (weight -> packed copy), and the
  // A-fragment-order copy of the norm2 output the step's out reduce writes for it
  std::map<const float*, const float*> fkmap_;
  float* hfrag_ = nullptr;
  // fused feed-forward of step passes (ffn_fused): linear2 fragment copies, the hand-off sets
  std::map<const float*, const float*> ffnmap_;
  float* ffn_hand_ = nullptr;
  int ffn_groups_ = 8;  // linear2 K slices (slabs) of the fused feed-forward
  int gemv_mask_ = 0;  // matrices that take the register-resident GEMM
  void derive_gemv();
  bool own_blob_ = true, ready_ = false;
  hipStream_t stream_ = nullptr;
  Layout L_{};
  float* blob_ = nullptr;
  std::vector<void*> allocs_, hallocs_;

  // per-slot streaming state (the FlowLM KV in fbm_, the codec's in bbm_)
  long ring_slot_ = 0, ring_layer_ = 0;
  int* fpos_ = nullptr;
  // shared voice prefixes (KvStore::pre): per slot, the voice cache its positions < F read from
  // and F (0: the slot's own rows); pinned host mirrors; the
  // voice each slot references. PTTS_NO_SHARED_VOICE (probe builds) copies the prefix in instead.
  bool share_voice_ = true;
  const float** vpre_ = nullptr;
  int* vlen_ = nullptr;
  const float** h_vpre_ = nullptr;
  int* h_vlen_ = nullptr;
  std::vector<const ptts_voice*> slot_voice_;
  // the slot lets go of its voice (freed here if it was destroyed meanwhile: `drained` = no queued
  // work may still read it, else stream_ is synchronized first)
  void voice_release(int slot, bool drained);
  SlotState* st_ = nullptr;
  float *lat_in_ = nullptr, *cur_ = nullptr, *eos_ = nullptr;
  int hist_T_[8] = {}, hist_C_[8] = {}, hist_P_[8] = {};

  // activations
  static constexpr int PREFILL = 2048;  // rows per prefill pass (batched admission: all slots' text)
  // split-tail scratch of the prefill GEMMs (GemmArgs::tail_S; one stream at a time uses it)
  static constexpr size_t TAIL_CAP = (size_t)16 << 20;
  static constexpr int TICKETS = 1024;
  int* ids_dev_ = nullptr;
  int* rowtab_dev_ = nullptr;   // [PREFILL] slot << 16 | pos, -1 = padding row (16-row groups)
  int *ctab_dev_ = nullptr, *qrow_dev_ = nullptr, *orow_dev_ = nullptr;  // compact admission rows (RowMap)
  int* admit_slots_ = nullptr;  // [max_slots] staged admission list
  SlotState* admit_st_ = nullptr;
  int* admit_fpos_ = nullptr;
  // latent prefixes (section 20): one pass's prefix latents [PREFILL][32], the admitted rows' first
  // backbone inputs [max_slots][32] and RESET_* bits [max_slots], each with its pinned staging
  float *plat_dev_ = nullptr, *h_plat_ = nullptr, *admit_lat_ = nullptr, *h_alat_ = nullptr;
  int *admit_opt_ = nullptr, *h_aopt_ = nullptr;
  float *ysilu_ = nullptr, *mods_ = nullptr, *xf_ = nullptr, *hf_ = nullptr, *uf_ = nullptr;
  // persistent flow-head chain (k_flow_head): hand-off rows, counters, timeout word
  bool head_uniform_stride() const;  // ResBlock tensors at one stride (k_flow_head, its packing)
  bool use_head_chain(int B) const;
  float* fhw_ = nullptr;  // the chain's matrices in fragment order (pack_flow_head, at finalize)
  float* hx_ = nullptr;   // flow-head hand-off regions [cap * 13][roundup(B, 16)][512] (k_flow_head)
  float* fhm_ = nullptr;  // adaLN shift / scale in k_flow_head's fragment order (FlowHeadArgs::fhm)
  float* fh_inw_t_ = nullptr;  // flow-head input projection transposed [32][512] (x0 side job)
  size_t hx_floats(int B) const { return hx_floats(B, lsd_); }
  size_t hx_floats(int B, int lsd) const { return (size_t)lsd * 13 * ((B + 15) / 16 * 16) * FD; }
  // flow-head prelude (head_prelude: f32 engines, B <= 32 on the chain): the cond | EOS matrix in
  // gemv_fk's order followed by the adaLN matrix in pack_head_ada's (finalize), and its hand-off
  // regions [cap][2][HP_REGION_FLOATS], emptied by the out_norm reduce ahead of it
  bool use_head_prelude(int B) const;
  float *hp_w_ = nullptr, *hp_hand_ = nullptr;
  float* inw_t_ = nullptr;  // input_linear weight transposed, [32][1024] (k_input_ln)
  int *hctr_ = nullptr, *herr_ = nullptr;
  float* trb_[3] = {};  // transposed-conv biases replicated over the r output phases [r][Cout]
  // front -> back hand-off per step parity, and the back part's own split-K slabs
  // Up to three hand-off buffers: front(k) writes buffer k % nhb_ and waits only for back(k - nhb_)
  // (nhb_ = 3 lets front and back drift a step apart instead of running in lockstep).
  // 3 nfr hand-off buffers with passes over nfr = back_frames > 1 frames: a pass's nfr buffers
  // are read while the fronts of the next 2 nfr frames fill the others (the front part may run two
  // passes ahead of the back part).
  static constexpr int NHB = NHB_MAX;
  int nhb_ = 3;  // buffers in use: 3, or 3 nfr with multi-frame passes
  int nfr_ = 1;  // frames per back-part pass (ptts_engine_config.back_frames)
  int back_mfma_ = PTTS_BACK_F32;  // ptts_engine_config.back_mfma: the back part's tiles' arithmetic
  // bf16x6 back part: weight matrix -> its split3 copy (hi | mid, lo), derive_split at finalize
  std::map<const float*, std::pair<const unsigned*, const unsigned short*>> split_;
  void derive_split();
  void attach_split(GemmArgs& a) const;
  int rows_hb_[NHB] = {};  // rows of the front part that filled each hand-off buffer
  // multi-frame passes: PCM of one pass [B][nfr][1920] followed by the meta blocks of its nfr
  // buffers, per pass (buffers q with q / nfr = p), and its pinned host copy
  float* pcmp_[NHB / 2] = {};
  float* h_pcmp_[NHB / 2] = {};
  // rows admitted inside a pass's calls (not at a call k with k % nfr == 0) start at the next pass
  // boundary: their SlotState (active) is written right before that front part (pinned staging)
  SlotState* h_act_ = nullptr;
  std::vector<int> act_slots_;
  int admit_delay_ = 0;
  // positions the attention ops' algorithmic costs are stated for (plan_names; 0 = a default):
  // the mean FlowLM context and Mimi window of the rows, and the FlowLM cached positions one step
  // attention launch reads (every row's own positions + each distinct shared voice prefix once)
  double plan_ctx_ = 0, plan_win_ = 0, plan_kvu_ = 0;
  float* lat_out_[NHB] = {};
  float* eos_out_[NHB] = {};
  FrameFlags* flags_[NHB] = {};
  float* pcm_[NHB] = {};
  float* meta_[NHB] = {};  // per parity, one allocation: lat_out [B][32] | flags [B] | eos_out [B]
  size_t meta_floats_ = 0;
  int back_cap_ = 1;  // max workgroups per CU of the pipelined back part's kernels (PTTS_BACK_WG_CAP: probe builds)
  // pipelined stepping (cfg.pipeline): back part on its own stream, parity events
  bool pipeline_ = false;
  hipStream_t stream_be_ = nullptr;
  hipEvent_t ev_front_[NHB] = {}, ev_back_[NHB] = {};
  // admission / slot_close / set_latent write slot state on stream_ after the last front part the
  // next back part decodes: that back part (stream_be_) waits for this event first
  hipEvent_t ev_admit_ = nullptr;
  hipEvent_t ev_be_tail_ = nullptr;  // stream_be_'s queue at an admission (stream_ waits for it)
  hipEvent_t ev_act_ = nullptr;      // after the latest start-of-utterance copies from h_act_
  bool admit_pending_ = false;
  void mark_admission();
  long long k_ = 0;          // steps issued
  int out_hb_ = 0;           // hand-off buffer of the frame the last call produced
  int out_rows_ = 0;         // rows that frame covers
  int prev_hb_ = 0, prev_rows_ = 0;  // the same for the call before (fetch with calls_back = 1)
  long long out_k_ = -1, prev_k_ = -1;  // the call index of those frames
  // per slot: the index of the first call of its current utterance (the admission's k_): a fetched
  // frame of an earlier call belongs to the slot's previous utterance and does not drain the slot
  std::vector<long long> admit_call_;
  // slots_cancel: slots whose current utterance was cancelled (until their next admission), and
  // the frames still to mask: calls [from, to) of `slot` belong to a cancelled utterance (from: its
  // admission's call index, to: the cancel's). Entries leave once no fetch can reach their calls.
  std::vector<char> cancelled_;
  struct CancelWin {
    int slot;
    long long from, to;
  };
  std::vector<CancelWin> cancel_wins_;
  bool frame_cancelled(int b, long long fk) const {
    for (const CancelWin& w : cancel_wins_)
      if (w.slot == b && fk >= w.from && fk < w.to) return true;
    return false;
  }
  SlotState* h_idle_ = nullptr;  // pinned, constant: the idle state (active 0, eos_step -1) slots_cancel copies in
  int front_rows_ = 0;       // rows of the last front part (0: the call was a flush)
  bool admitted_since_call_ = false;  // an admission since the last step / flush call
  // fbm_.x / fbm_.h / lat_in_ written outside the step graphs since the last front part (refresh_xh)
  bool xh_dirty_ = true;
  void refresh_xh();
  void call_async(int B, bool front);
  float *temb_ = nullptr, *temb_tmp_ = nullptr;
  float* rope_ = nullptr;  // FlowLM RoPE cos/sin table [max_ctx][32][2]

  // pinned host staging: each back graph ends in async D2H copies of its frame (PCM + metadata)
  // into the host set of its parity, so fetch() only reads host memory
  float* h_pcm_[NHB] = {};
  float* h_meta_[NHB] = {};
  int* h_err_ = nullptr;  // copy of herr_ made at the end of every front graph
  // probe builds (PTTS_STAMPS=path): realtime stamps at the start / end of every part graph,
  // written to the file at destruction (tools/stamps.py)
#ifdef PTTS_PROBES
  unsigned long long* stamp_ring_ = nullptr;
  unsigned* stamp_ctr_ = nullptr;
  std::vector<std::string> stamp_names_[2];  // op names of the stamped graphs (PTTS_STAMP_OPS)
#endif
  int head_resident_ = 0;  // k_flow_head workgroups that can be co-resident on this device
  int *h_slots_ = nullptr, *h_fp_ = nullptr, *h_ids_ = nullptr, *h_tab_ = nullptr;  // admission staging
  SlotState* h_st_ = nullptr;

  std::map<int, hipGraphExec_t> graphs_;
  std::map<int, hipGraph_t> graph_defs_;

  // slots whose utterance has no frame left in flight (never admitted, closed, or its last frame
  // fetched): their admission need not wait for the back parts already queued (ev_be_tail_)
  std::vector<char> drained_;
  // slots whose codec state is that of a whole utterance (never used, or its last frame fetched, and
  // neither closed nor cancelled since): the ones keep_codec may be admitted on
  std::vector<char> codec_ok_;

  // ---- first-frame previews (preview_enable)
  static constexpr int PV_MAX = 8;  // rows per preview pass (the small-tile back path: < 16 rows)
  static constexpr int PV_Q = 8;    // previews in flight / not yet fetched
  struct PvEntry {
    int n = 0;
    int slots[PV_MAX] = {};
    hipEvent_t ev = nullptr;
    float* h_pcm = nullptr;  // pinned [PV_MAX][1920]
  };
  int pv_max_ = 0;
  hipStream_t stream_pv_ = nullptr;
  // the preview passes' own workspace (its codec state stays the fresh one) and their compact batch
  BackBufs pv_{};
  float *pv_lat_ = nullptr, *pv_pcm_ = nullptr;
  FrameFlags* pv_flags_ = nullptr;
  PvEntry pv_q_[PV_Q];
  int pv_head_ = 0, pv_count_ = 0;  // FIFO of launched, unfetched previews
  std::vector<std::pair<int, long long>> pv_pending_;  // (slot, call of its first front part)
  hipEvent_t ev_pv_front_ = nullptr;
  hipEvent_t ev_call_[4] = {};  // after the front part (or flush) of call k: ev_call_[k % 4]
  // calls from this one on record ev_call_ (set by the first front_done(): a caller that never
  // asks puts no event marker on the front stream per call); -1 = none yet
  long long call_ev_from_ = -1;
  hipEvent_t ev_pv_read_[NHB] = {};  // a preview's gather of hand-off buffer q (front(q + nhb) waits)
  bool pv_read_pending_[NHB] = {};
  std::map<int, hipGraphExec_t> pv_graphs_;
  std::map<int, hipGraph_t> pv_graph_defs_;
  void launch_previews(int B, int hb);
  hipGraphExec_t pv_graph(int P);
  void pv_forget(int slot);  // drop the slot's pending / unfetched previews (re-admitted or closed)

  // ---- wire stage (wire_enable)
  bool wire_ = false;
  int* wire_fmt_ = nullptr;     // [max_slots] encoding | rate index << 8 (0: none)
  std::vector<int> slot_wire_;  // its host mirror (copy_out: no chunk copy while no row has a format)
  int* wire_frames_ = nullptr;  // [max_slots] frames received
  float* wire_tail_ = nullptr;  // [max_slots][WIRE_TAIL]
  float* wire_taps_ = nullptr;
  WirePlan wire_plan_[WIRE_RATES] = {};
  int* admit_wire_ = nullptr;   // staged formats of an admission (device), h_wire_ (pinned)
  int* h_wire_ = nullptr;
  // ---- tempo stage (tempo_enable): per-row speed and state, back-owned like the wire state
  bool tempo_ = false;
  int* tempo_sp_ = nullptr;      // [max_slots] permille (0: none)
  int* tempo_state_ = nullptr;   // [max_slots][TEMPO_STATE]
  float* tempo_hist_ = nullptr;  // [max_slots][TEMPO_HIST]
  float* tempo_win_ = nullptr;   // [TEMPO_W]
  float* tempo_out_ = nullptr;   // [max_slots][nfr][TEMPO_OUT_MAX]: one pass's chunks (k_tempo -> k_wire)
  int* tempo_cnt_ = nullptr;     // [max_slots][nfr]
  int* admit_tempo_ = nullptr;   // staged speeds of an admission (device), h_tempo_ (pinned)
  int* h_tempo_ = nullptr;
  // ---- pitch stage (pitch_enable): per-row step and state, back-owned like the tempo state
  bool pitch_ = false;
  unsigned* pitch_step_ = nullptr;  // [max_slots] Q20 input samples per output sample (0: none)
  int* pitch_state_ = nullptr;      // [max_slots][PITCH_STATE]
  float* pitch_hist_ = nullptr;     // [max_slots][PITCH_HIST]
  float* pitch_tab_ = nullptr;      // [PITCH_TAB][2]
  float* pitch_out_ = nullptr;      // [max_slots][nfr][PITCH_OUT_MAX]: one pass's chunks (k_pitch -> k_wire)
  int* pitch_cnt_ = nullptr;        // [max_slots][nfr]
  unsigned* admit_pitch_ = nullptr; // staged steps of an admission (device), h_pitch_ (pinned)
  unsigned* h_pitch_ = nullptr;
  // ---- level stage (level_enable): per-row gain and state, back-owned like the tempo state
  bool level_ = false;
  float level_ceiling_ = 1.f;       // the engine's ceiling (level_plan)
  unsigned* level_gain_ = nullptr;  // [max_slots] f32 bits of the row's gain (0: not in the stage)
  int* level_state_ = nullptr;      // [max_slots][LEVEL_STATE]
  float* level_hist_ = nullptr;     // [max_slots][LEVEL_HIST]
  float* level_out_ = nullptr;      // [max_slots][nfr][LEVEL_OUT_MAX]: one pass's chunks (k_level -> k_wire)
  int* level_cnt_ = nullptr;        // [max_slots][nfr]
  unsigned* admit_level_ = nullptr; // staged gains of an admission (device), h_level_ (pinned)
  unsigned* h_level_ = nullptr;
  // ---- loudness stage (loud_enable): per-row state, back-owned like the level state
  bool loud_ = false;
  LoudCoef loud_coef_{};
  int* loud_state_ = nullptr;     // [max_slots][LOUD_STATE]
  float* loud_pend_ = nullptr;    // [max_slots][LOUD_SUB]
  double* loud_filt_ = nullptr;   // [max_slots][LOUD_FILT]
  int* admit_loud_ = nullptr;     // staged flags of an admission (device), h_loud_ (pinned)
  int* h_loud_ = nullptr;
  // ---- FLAC stage (flac_enable)
  bool flac_ = false;
  int* flac_first_ = nullptr;    // [max_slots][nfr] a FLAC chunk's first sample index (k_wire -> k_flac)
  // per pass (index: hand-off buffer / frames per pass): counts [max_slots][nfr] | on a FLAC-enabled
  // engine the chunks' frame counts [max_slots][nfr] and frame index [max_slots][nfr][3][2] | chunks
  // [max_slots][nfr][WIRE_CHUNK_MAX], and its pinned host copy
  static constexpr int WIRE_BLOCKS = 3;
  unsigned char* wireb_[WIRE_BLOCKS] = {};
  unsigned char* h_wireb_[WIRE_BLOCKS] = {};
  // the head: byte counts | (FLAC: frame counts | index) | (loudness: a LoudRecord per (row, frame))
  size_t wire_loud_off() const {
    return ((size_t)max_slots_ * nfr_ * sizeof(int) * (flac_ ? 2 + 2 * FLAC_CHUNK_FRAMES : 1) + 15) / 16 * 16;
  }
  size_t wire_head_bytes() const {
    const size_t ints = (size_t)max_slots_ * nfr_ * sizeof(int) * (flac_ ? 2 + 2 * FLAC_CHUNK_FRAMES : 1);
    return ((loud_ ? wire_loud_off() + (size_t)max_slots_ * nfr_ * sizeof(LoudRecord) : ints) + 127) / 128 * 128;
  }
  void wire_blocks_alloc();  // new pass blocks of the current head and chunk sizes (the old ones stay until destruction)
  size_t wire_block_bytes(int rows) const { return wire_head_bytes() + (size_t)rows * nfr_ * wire_chunk_max(); }
  static int wire_rate_index(int rate);

  // ---- align stage (align_enable): front-owned, one FlowLM layer
  bool align_ = false;
  int align_layer_ = 0;
  unsigned align_mask_ = 0;
  AlignEntry* align_tab_ = nullptr;    // [max_slots] {first text position, tokens} (n == 0: not in the stage)
  AlignEntry* h_align_src_ = nullptr;  // pinned staging of one admission's entries
  std::vector<int> slot_align_;        // host mirror of the entries' n
  float* alignb_ = nullptr;            // [NHB][max_slots][ALIGN_ROW]: hand-off buffer q's rows
  float* h_alignb_ = nullptr;          // pinned copy
  // per hand-off buffer: a row of the front part that filled it was in the stage (copy_out copies
  // the buffer's block, fetch_align reads it)
  bool align_any_[NHB] = {};
  float* align_block(int hb) const { return alignb_ + (size_t)hb * max_slots_ * ALIGN_ROW; }

  // ---- voice cloning: everything a clone writes but the voice itself lives in a VoiceWs, so a
  // clone shares only read-only weights and tables with the step pipeline
  struct VoiceWs {
    int frames = 0;         // capacity in frames of `block`
    size_t up_bytes = 0;    // capacity of the device block `up` (the upload, then the converted clip)
    size_t h_bytes = 0;     // capacity of each pinned staging block (0: none, synchronous clones)
    // one upload per clone: raw samples | resampler taps | rubato start / frac tables (behind them on
    // the device, rubato rule only: the converted samples [n_in]); a prompt's rows go straight into
    // fb.x. Jobs stage it in one of two pinned host blocks (h_up; ev_up: that block's latest upload has run)
    char* up = nullptr;
    char* h_up[2] = {};
    hipEvent_t ev_up[2] = {};
    float* block = nullptr;                    // one allocation holding everything below
    float *pcm = nullptr;                      // frame-padded 24 kHz input [Np]
    float *A = nullptr, *Bf = nullptr, *V = nullptr, *zeros = nullptr;  // SEANet encoder ping-pong, zero history
    float *eh = nullptr, *eqkv = nullptr, *eq = nullptr, *eo = nullptr, *eu = nullptr, *ering = nullptr;
    float *Hd = nullptr, *lat = nullptr, *cond = nullptr;
    FlowBufs fb{};                             // the prompt prefill's x, h, q, o, u, slabs, tail scratch
  };
  static void vws_free(VoiceWs& w);  // everything vws_reserve allocated
  static void vws_reserve(VoiceWs& w, hipStream_t st, int frames, size_t host_bytes, size_t up_bytes);
  ptts_voice* voice_new(int F, bool pcm, bool job);
  void voice_clone(const VoicePlan* p, const VoiceWs& w, hipStream_t st, ptts_voice* v, float* h_cond);
  ptts_voice* voice_sync(const VoicePlan* p, const void* src, int F);
  VoiceWs vws_{};                    // the jobs' grow-only workspace
  hipStream_t stream_vc_ = nullptr;  // lowest priority; plain launches of non-persistent kernels only
  long long vjobs_ = 0;              // jobs started (upload block parity)
  void vjob_reserve(int frames, size_t host_bytes, size_t up_bytes);
  ptts_voice* voice_job(const VoicePlan* p, const void* src, int F);
};

}  // namespace ptts
