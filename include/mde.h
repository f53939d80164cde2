/*
 * mde.h -- C ABI of libmde_hip.so, the MI355X (gfx950) monocular depth
 * inference engine (Depth Anything V2 family; Depth Pro).  Plain pointers, sizes and ints only: no torch, no HIP
 * C++ types (streams/events are opaque `void*` = hipStream_t / hipEvent_t).
 *
 * Every function returns 0 (MDE_OK) on success or an mde_status code;
 * mde_last_error() returns a thread-local description of the last failure.
 *
 * Which reference interface each group replaces (reference paths are
 * relative to the upstream repo yester31/Monocular_Depth_Estimation_TRT):
 *
 *   engine        core/common.py:141-312 get_engine() -> trt.ICudaEngine
 *                 (deserialize_cuda_engine, :298-299) and its introspection
 *                 used by core/common_runtime.py:131-175 (num_io_tensors,
 *                 get_tensor_name/shape/dtype/mode, get_tensor_profile_shape)
 *                 Depth Pro: models/depth_pro/onnx2trt.py:94-111 (same engine API,
 *                 outputs "canonical_inverse_depth" + "fov_deg", onnx_export.py:56)
 *                 VGGT: models/vggt/onnx2trt.py:95-107 (input "images" [1,S,3,518,518],
 *                 output "depth", onnx_export.py:125-127)
 *   context       engine.create_execution_context()
 *                 (models/depth_anything_v2/onnx2trt.py:93-94),
 *                 context.set_tensor_address (core/common_runtime.py:272-274),
 *                 context.set_input_shape (onnx2trt.py:99-100),
 *                 context.execute_async_v3 (core/common_runtime.py:269-270),
 *                 context.profiler = IProfiler (tools/profile_model.py:126,
 *                 core/profile.py:30-57)
 *   rt            the cuda-python cudart calls of core/common_runtime.py
 *                 (cudaMallocHost/cudaMalloc :64-73, cudaFree/cudaFreeHost
 *                 :106-108, cudaMemcpyAsync :245-255, cudaStreamCreate/
 *                 Synchronize/Destroy :135,:259,:182, cudaEvent* :220-237)
 *   op            no reference counterpart: the individual TensorRT layers of
 *                 the DA-V2 engine, exposed for per-kernel
 *                 parity tests and for integrators who run parts of the graph.
 */
#ifndef MDE_H_
#define MDE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDE_ABI_VERSION 12

typedef enum {
  MDE_OK = 0,
  MDE_ERR_ARG = 1,     /* bad argument (null pointer, bad size)          */
  MDE_ERR_FILE = 2,    /* packed file missing or unreadable              */
  MDE_ERR_FORMAT = 3,  /* packed file malformed / unsupported version    */
  MDE_ERR_HIP = 4,     /* HIP runtime error                              */
  MDE_ERR_NAME = 5,    /* unknown tensor name                            */
  MDE_ERR_SHAPE = 6,   /* shape outside the engine's profile             */
  MDE_ERR_STATE = 7    /* address not set, context busy, ...             */
} mde_status;

/* Same numbering as tensorrt.DataType for the types used here. */
typedef enum { MDE_FLOAT32 = 0, MDE_FLOAT16 = 1, MDE_UINT8 = 5 } mde_dtype; /* tensorrt.DataType values */

typedef struct mde_engine mde_engine;
typedef struct mde_context mde_context;

typedef struct {
  char name[64];
  int32_t dtype;    /* mde_dtype */
  int32_t is_input; /* 1 = INPUT, 0 = OUTPUT (trt.TensorIOMode) */
  int32_t rank;
  int64_t dims[8];  /* dims[0] = -1: batch is dynamic (see profile shape) */
} mde_io_desc;

typedef struct {
  char encoder[16];
  int32_t embed_dim, depth, num_heads, mlp_hidden, patch;
  int32_t img_h, img_w, features, head_hidden, metric;
  int32_t out_channels[4], taps[4];
  float max_depth, ln_eps;
  int32_t max_batch_hint;
  int64_t weight_bytes;
  int32_t input_format; /* 0: "input" float32 NCHW [B,3,H,W]; 1: "image_u8" uint8 NHWC [B,H,W,3] */
  int32_t family;       /* 0: Depth Anything V2 (io "input" -> "output" [B,H,W]);
                           1: Depth Pro (io "input" [B,3,1536,1536] -> "canonical_inverse_depth"
                              [B,1,1536,1536] and, with the FOV head, "fov_deg" [B]);
                           2: VGGT depth path (io "images" float32 [B,S,3,H,W] in [0,1] ->
                              "depth" [B,S,H,W,1]; S fixed at pack time) */
} mde_engine_info;

/* IProfiler.report_layer_time analogue: one call per launched layer. */
typedef void (*mde_layer_cb)(const char* layer_name, float ms, void* user);

/* ---- library ---------------------------------------------------------- */
int mde_version(void);
const char* mde_last_error(void);
/* Dispatch switches (no reference counterpart: TensorRT picks tactics at build
 * time).  Each starts at its default, is overridden once per process from the
 * environment variable MDE_<NAME>, and can be changed here afterwards; a
 * captured hipGraph keeps the choice it was captured with.  Names (range,
 * default): "splitk" (0-1, 1) split-K of small-grid GEMMs / DPT convs;
 * "lnfold" (0-1, 1) LayerNorm folded into the consumer GEMMs, read at context
 * creation; "conv_narrow" (0-1, 1) narrow conv channel tiles on small grids;
 * "upconv" (0-1, 1) separable upsampling head conv; "gemm256" (0-2, 1) 256^2
 * GEMM tiles (0 never, 1 auto, 2 always); "deep64" (0-1, 1) 4-deep ring for
 * small-grid 64^2 tiles; "w8small" (0-1, 1) 8-wave small-grid 128^2 tiles;
 * "conv_persist" (0-2, 1) persistent 64-channel RCU conv (1: 16 x 16 tiles,
 * 2: 8 x 16); "panel" (0-2, 1) A-stationary panel GEMM for the K = 384
 * qkv / fc1 at large batch (2: also the f16-residual proj); "panel32" (0-1,
 * 0) that GEMM on 32x32x16 MFMAs with the LN fold's mean term in the
 * accumulator's initial value (within 1 f16 ulp of the default); "narrow_resid"
 * (0-1, 1) 32 x 64 whole-K tiles for small-grid residual updates instead of
 * split-K + reduce; "attn16" (0-1, 1) the large-grid attention on 16x16x32
 * MFMAs (same softmax, other summation grouping); "splitk_fused" (0-1, 0) the
 * engines' split-K slices and their in-order reduce as one launch (the last
 * slice of a tile to arrive adds the slots; measured slower); "attn_tail" (0-2, 2)
 * the large-grid attention's partial query blocks dispatched after the full
 * ones (1: work order only, bit-identical; 2: those blocks also split their
 * keys over two wave groups); "resize_fold" (0-1, 1) the DPT fusion blocks' x2
 * resize read on the fly by the next block's residual conv (bit-identical);
 * "outconv_fold" (0-1, 1) the DPT fusion blocks' 1x1 out_conv run inside the
 * persistent RCU conv in front of it (bit-identical).  The environment variable of a switch is exactly
 * MDE_ + its name upper-cased (MDE_DEEP64, MDE_W8SMALL, ...); a value that is
 * not an integer in range is reported on stderr and ignored.
 * Every setting computes the same depth map within the stated tolerance; the
 * tile switches are bit-identical.  MDE_ERR_NAME: unknown name; MDE_ERR_ARG:
 * value out of range. */
int mde_tuning_set(const char* name, int value);
int mde_tuning_get(const char* name, int* value);
/* For tests and tools: the route the calling thread's last GEMM-family launch
 * (every mde_op_linear*, qkv*, conv3x3*, conv_transpose*, patch_embed and
 * depth_head* op, and each such layer of an enqueue) took, as one line of
 * key=value fields, e.g. "kind=tile bm=128 bn=128 wm=2 wn=2 bk=32 stages=3
 * slices=1 fused=0 resize_first=0".  kind: none (nothing launched yet, or an
 * empty problem), tile, split_store, split_resid (these three with every
 * field: block tile, wave grid, K-step, LDS ring depth, split-K slices, fused
 * split tail, a resize launch in front), conv_direct ("kind=conv_direct
 * conv=upconv resize_first=0": conv names the kernel of conv.hip that ran --
 * conv3 the per-tile direct conv, conv3_up the same kernel with its four-tap
 * upsampling loader, upconv / upconv_persist the separable upsampling conv
 * with one tile per workgroup / on its persistent grid, conv64p the
 * persistent 64-channel conv -- and resize_first), panel, gemm256.  A reader
 * takes the fields by name: later versions may add some.  MDE_ERR_ARG: null
 * buffer, or n too small (128 suffices). */
int mde_debug_last_gemm_route(char* buf, size_t n);
/* The same for the calling thread's last f16 attention launch
 * (mde_op_attention, _ws, _cfg, and each attention layer of an enqueue; the
 * fp32 op has the record below): what was launched after every
 * fall-back of the launcher, e.g. "kernel=mfma32 nw=8 groups=4 split=1 tiles=0
 * ring=2 qs=1 tail=0 nqb=22 nkt=22".  kernel: none (nothing launched yet, an
 * empty problem, or a call rejected with MDE_ERR_ARG -- no other field then), mfma32 (the 32x32x16 kernel),
 * mfma16 (the 16x16x32 kernel); nw waves per workgroup; groups key groups
 * inside the workgroup (1: none -- also when a forced count exceeds the key
 * tiles); split the key splits over the grid that were launched, with the
 * combine kernel behind them (1: none -- also when the split collapsed or the
 * workspace was too small) and tiles the key tiles of each; ring the K / V^T
 * ring depth; qs the 32-query sub-tiles per wave; tail the "attn_tail" switch
 * handed to the mfma16 kernel (0 for mfma32); nqb query blocks per (sequence,
 * head); nkt 64-key tiles.  Fields by name, errors and n as above. */
int mde_debug_last_attention_route(char* buf, size_t n);
/* And for the fp32 attention (mde_op_attention32, the fp32 engines' attention
 * layers): "kernel=fp32 key_groups=4 nqb=43" -- key_groups 4: four waves share
 * one 32-query block and a quarter of the keys each (small grids); 1: four
 * 32-query blocks per workgroup over all keys; nqb query blocks per
 * (sequence, head) -- or "kernel=none" as above. */
int mde_debug_last_attention32_route(char* buf, size_t n);

/* ---- engine (replaces get_engine / ICudaEngine) ----------------------- */
int mde_engine_load(const char* packed_path, int device, mde_engine** out);
int mde_engine_load_memory(const void* data, size_t nbytes, int device, mde_engine** out);
int mde_engine_destroy(mde_engine* eng);
int mde_engine_get_info(const mde_engine* eng, mde_engine_info* out);
int mde_engine_num_io(const mde_engine* eng, int* n);
int mde_engine_io_desc(const mde_engine* eng, int index, mde_io_desc* out);
/* which: 0 = min, 1 = opt, 2 = max shape of the dynamic-batch profile */
int mde_engine_profile_shape(const mde_engine* eng, const char* name, int which, int64_t* dims, int* rank);

/* ---- execution context (replaces IExecutionContext) ------------------- */
int mde_context_create(mde_engine* eng, int max_batch, mde_context** out);
int mde_context_destroy(mde_context* ctx);
int mde_context_set_tensor_address(mde_context* ctx, const char* name, void* device_ptr);
int mde_context_set_input_shape(mde_context* ctx, const char* name, const int64_t* dims, int rank);
int mde_context_get_tensor_shape(const mde_context* ctx, const char* name, int64_t* dims, int* rank);
/* Asynchronous: enqueues the whole forward on `stream` (hipStream_t). */
int mde_context_enqueue(mde_context* ctx, void* stream);
/* 1 (default): capture the forward into a hipGraph per (batch, addresses)
 * and replay it; 0: launch every kernel eagerly. */
int mde_context_set_graph_mode(mde_context* ctx, int enable);
/* Non-null cb: enqueue runs eagerly with a hipEvent pair per layer,
 * synchronizes `stream` at the end and reports each layer's time. */
int mde_context_set_profiler(mde_context* ctx, mde_layer_cb cb, void* user);
int mde_context_workspace_bytes(const mde_context* ctx, size_t* bytes);

/* ---- HIP runtime helpers (replaces cuda-python cudart) ---------------- */
int mde_rt_device_count(int* n);
int mde_rt_set_device(int device);
int mde_rt_device_name(int device, char* buf, int buflen);
int mde_rt_malloc(void** ptr, size_t bytes);
int mde_rt_free(void* ptr);
int mde_rt_malloc_host(void** ptr, size_t bytes);
int mde_rt_free_host(void* ptr);
int mde_rt_memcpy_htod_async(void* dst, const void* src, size_t bytes, void* stream);
int mde_rt_memcpy_dtoh_async(void* dst, const void* src, size_t bytes, void* stream);
int mde_rt_memcpy_dtod_async(void* dst, const void* src, size_t bytes, void* stream);
int mde_rt_memset_async(void* dst, int value, size_t bytes, void* stream);
int mde_rt_stream_create(void** stream);
int mde_rt_stream_destroy(void* stream);
int mde_rt_stream_synchronize(void* stream);
int mde_rt_device_synchronize(void);
int mde_rt_event_create(void** event);
int mde_rt_event_destroy(void* event);
int mde_rt_event_record(void* event, void* stream);
int mde_rt_event_elapsed_ms(float* ms, void* start, void* end);

/* ---- kernel-level entry points ---------------------------------------- */
/* All tensors are device pointers.  f16 = IEEE half.  Weights W are
 * [Npad][ldw] f16 row-major (K contiguous), rows >= N zero, ldw % 64 == 0,
 * ldw >= K rounded up to 64, Npad a multiple of 128; N % 8 == 0.  Activation maps are
 * NHWC f16.  act: 0 none, 1 ReLU, 2 GELU(erf). */
/* The same over an f16 residual stream (precision "fp16" engines): x_f16 [rows][dim]. */
int mde_op_layernorm_f16(const void* x_f16, void* y_f16, const float* gamma, const float* beta, int rows, int dim,
                         float eps, int tokens, int skip_cls, void* stream);
int mde_op_layernorm(const float* x, void* y_f16, const float* gamma, const float* beta, int rows, int dim,
                     float eps, int tokens, int skip_cls, void* stream);
int mde_op_linear(const void* a_f16, int lda, const void* w_f16, int ldw, int m, int n, int k,
                  const float* bias, int act, void* out_f16, int ldo, void* stream);
int mde_op_linear_residual(const void* a_f16, int lda, const void* w_f16, int ldw, int m, int n, int k,
                           const float* bias, const float* layer_scale, float* x32, int ldx, void* stream);
int mde_op_qkv(const void* a_f16, const void* w_f16, int ldw, const float* bias, int batch, int tokens,
               int heads, int tokens_pad, float q_scale, void* q_f16, void* k_f16, void* vt_f16, void* stream);
/* mde_op_linear_residual over an f16 residual stream xh [m][ldx] (precision "fp16" engines):
 * xh += layer_scale * (a W^T + bias), one rounding to f16.  ln_partials (optional, n % 32 == 0):
 * fp32 [n/32][m][2] (slice-major) = per 32-column slice and row, the sum of the f16 values written
 * and their squared deviations from the slice mean -- the producer half of the folded LayerNorm (reference: the norm1 / norm2 after every
 * residual add of the DINOv2 blocks, upstream Block.forward). */
int mde_op_linear_residual_f16(const void* a_f16, int lda, const void* w_f16, int ldw, int m, int n, int k,
                               const float* bias, const float* layer_scale, void* xh_f16, int ldx, float* ln_partials,
                               void* stream);
/* The consumer half: out = act(LayerNorm(x) W^T + b) computed as act(rstd * (x Wg^T - mean * c1) + c2)
 * over the raw f16 rows x [m][k] (k % 32 == 0), with Wg = W * gamma (column k scaled by gamma[k]),
 * c1[n] = sum_k Wg[n][k], c2 = b + W beta, and mean / rstd (fp32, eps) from ln_partials [k/32][m][2] (k <= 1024). */
int mde_op_linear_lnfold(const void* x_f16, const float* ln_partials, float eps, const void* wg_f16, int ldw,
                         const float* c1, const float* c2, int m, int n, int k, int act, void* out_f16, int ldo,
                         void* stream);
/* mde_op_qkv with the LayerNorm folded in the same way (the DA-V2 engines' block qkv: norm1 ->
 * qkv, reference depth_anything_v2/dinov2_layers/block.py attn(norm1(x))): x [batch*tokens][64 heads]
 * raw f16 rows, ln_partials [heads*2][batch*tokens][2], wg = W * gamma, c1 / c2 as above. */
int mde_op_qkv_lnfold(const void* x_f16, const float* ln_partials, float eps, const void* wg_f16, int ldw,
                      const float* c1, const float* c2, int batch, int tokens, int heads, int tokens_pad,
                      float q_scale, void* q_f16, void* k_f16, void* vt_f16, void* stream);
/* q pre-multiplied by dh^-0.5 * log2(e) (scores in log2 units, as mde_op_qkv writes with
 * q_scale = 0.125 * log2(e)); k/q [B*H][tokens_pad][64], vt [B*H][64][tokens_pad] with key t
 * stored at column vt_pos(t) = t with bits 2 and 3 swapped, (t & ~12) | (t & 4) << 1 | (t & 8) >> 1
 * (the layout mde_op_qkv writes); ldo % 8 == 0 and o 16-B aligned. */
int mde_op_attention(const void* q_f16, const void* k_f16, const void* vt_f16, void* o_f16, int batch, int heads,
                     int tokens, int tokens_pad, int ldo, void* stream);
/* The same with an fp32 workspace for the split-KV path the launcher takes when the (head, query
 * block) grid is too small to fill the chip (batch 1); mde_op_attention_ws_bytes gives its size. */
int mde_op_attention_ws(const void* q_f16, const void* k_f16, const void* vt_f16, void* o_f16, int batch, int heads,
                        int tokens, int tokens_pad, int ldo, void* ws, size_t ws_bytes, void* stream);
size_t mde_op_attention_ws_bytes(int batch, int heads, int tokens);
/* mde_op_attention_ws with an explicit launch configuration (tests / tuning; no reference
 * counterpart): cfg = "<waves>[s<split>][g<groups>][r<ring>][q2][m]", e.g. "8" (256-query
 * workgroups), "8m" (the same on 16x16x32 MFMAs, unsplit 4 / 8 waves only), "4s2" (split-KV over two workgroups + merge kernel, needs ws), "4g2" (two key
 * groups of 64 queries inside one workgroup, merged through LDS); NULL or "" = the launcher's
 * policy. */
int mde_op_attention_cfg(const void* q_f16, const void* k_f16, const void* vt_f16, void* o_f16, int batch, int heads,
                         int tokens, int tokens_pad, int ldo, const char* cfg, void* ws, size_t ws_bytes,
                         void* stream);
/* Exact-fp32 kernels of precision "fp32" engines (fp32.hip; v_mfma_f32_16x16x4_f32 /
 * v_mfma_f32_32x32x2_f32, fp32 operands and accumulation): weights fp32 [Npad][ldw] (ldw % 32 == 0,
 * zero padded, Npad a multiple of 128), activations fp32 with lda % 4 == 0.  linear32: out = act(a w^T
 * + bias); linear_residual32: x32 += layer_scale * (a w^T + bias); qkv32: q (times q_scale) / k / v
 * fp32 [batch*heads][tokens_pad][64]; attention32: softmax over those (q pre-scaled by dh^-0.5 *
 * log2 e) -> o fp32 [batch*tokens][ldo]. */
int mde_op_linear32(const float* a, int lda, const float* w, int ldw, int m, int n, int k, const float* bias, int act,
                    float* out, int ldo, void* stream);
int mde_op_linear_residual32(const float* a, int lda, const float* w, int ldw, int m, int n, int k,
                             const float* bias, const float* layer_scale, float* x32, int ldx, void* stream);
int mde_op_qkv32(const float* a, const float* w, int ldw, const float* bias, int batch, int tokens, int heads,
                 int tokens_pad, float q_scale, float* q, float* k, float* v, void* stream);
int mde_op_attention32(const float* q, const float* k, const float* v, float* o, int batch, int heads, int tokens,
                       int tokens_pad, int ldo, void* stream);
/* The exact-fp32 DPT head's kernels (fp32.hip; precision "fp32" engines since ABI 7).  conv3x3_32: out
 * = act(conv3x3(relu_in ? ReLU(in) : in) + bias) + res0 + res1 over fp32 NHWC maps [batch][h][w][cin]
 * (cin % 4 == 0), pad 1, stride 1 or 2, weights fp32 [cout_pad][ldw] in (ky, kx, ci) order (ldw % 32
 * == 0, >= 9 cin rounded up to 32; cout % 4 == 0), res0 / res1 optional maps shaped like out --
 * reference: DPTHead's resConfUnit / layerN_rn / output_conv convs (upstream dpt.py), the reference's
 * fp32 TensorRT build (core/common.py:141-144).  conv_transpose32: ConvTranspose2d(k = s = stride)
 * as a GEMM with a pixel-shuffle epilogue, weights [(dy s + dx) cout + co][ldw] -- DPTHead
 * resize_layers 0/1.  resize32: bilinear, align_corners=True, fp32 NHWC (c % 4 == 0) --
 * F.interpolate in FeatureFusionBlock / the head. */
int mde_op_conv3x3_32(const float* in, int batch, int h, int w, int cin, const float* wt, int ldw, int cout,
                      int stride, int relu_in, const float* bias, int act, const float* res0, const float* res1,
                      float* out, void* stream);
int mde_op_conv_transpose32(const float* in, int batch, int h, int w, int cin, const float* wt, int ldw, int cout,
                            int stride, const float* bias, float* out, void* stream);
int mde_op_resize32(const float* in, int batch, int h, int w, int c, int oh, int ow, float* out, void* stream);
int mde_op_patch_embed(const float* img, int batch, int h, int w, const void* w_f16, int ldw, const float* bias,
                       const float* pos_patch, const float* cls_pos, int dim, void* patch_scratch_f16,
                       float* x32, void* stream);
int mde_op_conv3x3(const void* in_f16, int batch, int h, int w, int cin, const void* w_f16, int ldw, int cout,
                   int stride, int relu_in, const float* bias, int act, const void* res0_f16,
                   const void* res1_f16, void* out_f16, void* stream);
/* mde_op_conv3x3 / mde_op_linear (E_STORE) with an fp32 split-K workspace of
 * ws_floats elements: grids too small to fill the chip cut the K loop into
 * slices (partials summed in slice order, then the epilogue); *slices (may be
 * null) receives the slice count taken, 1 = no split.  The engine gives its
 * DPT convs such a workspace (small batches). */
int mde_op_conv3x3_ws(const void* in_f16, int batch, int h, int w, int cin, const void* w_f16, int ldw, int cout,
                      int stride, int relu_in, const float* bias, int act, const void* res0_f16,
                      const void* res1_f16, void* out_f16, float* ws, size_t ws_floats, int* slices, void* stream);
int mde_op_linear_ws(const void* a_f16, int lda, const void* w_f16, int ldw, int m, int n, int k, const float* bias,
                     int act, void* out_f16, int ldo, float* ws, size_t ws_floats, int* slices, void* stream);
int mde_op_conv3x3_up(const void* in_f16, int batch, int sh, int sw, int cin, int uh, int uw, const void* w_f16,
                      int ldw, int cout, const float* bias, int act, void* out_f16, void* stream);
int mde_op_conv_transpose(const void* in_f16, int batch, int h, int w, int cin, const void* w_f16, int ldw,
                          int cout, int stride, const float* bias, void* out_f16, void* stream);
int mde_op_resize_bilinear(const void* in_f16, int batch, int ih, int iw, int c, int oh, int ow, void* out_f16,
                           void* stream);
int mde_op_depth_head(const void* in_f16, int batch, int sh, int sw, int cin, int uh, int uw, const void* w_f16,
                      int ldw, const float* bias, const float* w2, float b2, int metric, float max_depth,
                      float* out_f32, void* stream);
/* ---- since ABI 11: the GEMM / conv options that only the engine graphs set, one thin test surface
 * each (no reference counterpart; tests/test_gpu_ops_engine_paths.py).  No policy of their own: the
 * launcher picks the route exactly as it does for the engines.
 *
 * Fused split-K operands, shared by three of them: tile_cnt (optional) = tile_cnt_cap zero-initialised
 * int counters, at least one per 64 x 64 output tile, left zero by every call; slot_floats = the part of
 * ws (<= ws_floats) the one-launch form may use for its per-tile slots.  With the switch "splitk_fused"
 * on and room for slices x tiles x tile area floats the split runs as one launch, otherwise as slices +
 * a reduce kernel -- the same sums in the same order. */
/* mde_op_linear_ws plus the E_STORE residual options: out = act(a W^T + bias) + r0 + res1, where r0 =
 * res0[m] (res0_rows == 0: res0 is [m][ldo]) or res0[m % res0_rows] (res0 is a [res0_rows][ldo] table,
 * VGGT's per-image positional embedding), through a ReLU when res0_relu (VGGT's in-place-ReLU residual
 * units).  res0 and res1 use the output's row stride ldo. */
int mde_op_linear_res(const void* a_f16, int lda, const void* w_f16, int ldw, int m, int n, int k, const float* bias,
                      int act, const void* res0_f16, int res0_rows, int res0_relu, const void* res1_f16,
                      void* out_f16, int ldo, float* ws, size_t ws_floats, int* slices, int* tile_cnt,
                      int tile_cnt_cap, size_t slot_floats, void* stream);
/* mde_op_conv3x3_ws plus res0_relu and res1_up: with res1_up_f16 [batch][res1_uh][res1_uw][cout] set,
 * res1 is its bilinear (align_corners=True) upsample to the output map -- read on the fly by the
 * direct conv's epilogue (switch "resize_fold"), or first written into res1_f16, which must be a
 * buffer of the output's shape either way. */
int mde_op_conv3x3_res(const void* in_f16, int batch, int h, int w, int cin, const void* w_f16, int ldw, int cout,
                       int stride, int relu_in, const float* bias, int act, const void* res0_f16, int res0_relu,
                       const void* res1_f16, const void* res1_up_f16, int res1_uh, int res1_uw, void* out_f16,
                       float* ws, size_t ws_floats, int* slices, int* tile_cnt, int tile_cnt_cap, size_t slot_floats,
                       void* stream);
/* mde_op_linear_lnfold reading the residual stream past every sequence's cls row (the DPT projects):
 * x [seqs*tokens][k] and ln_partials [k/32][seqs*tokens][2] cover all rows, out has seqs*(tokens-1)
 * rows; output row r reads row (r / (tokens-1)) * tokens + 1 + r % (tokens-1).  tokens >= 2. */
int mde_op_linear_lnfold_tok(const void* x_f16, const float* ln_partials, float eps, const void* wg_f16, int ldw,
                             const float* c1, const float* c2, int seqs, int tokens, int n, int k, int act,
                             void* out_f16, int ldo, void* stream);
/* mde_op_depth_head with hpe_f16 (optional) [hpe_pix][32] added to the hidden layer before its ReLU at
 * output pixel m % hpe_pix (VGGT: the folded conv of the UV positional embedding).  metric: 0 ReLU,
 * 1 max_depth * sigmoid, 2 exp. */
int mde_op_depth_head_pe(const void* in_f16, int batch, int sh, int sw, int cin, int uh, int uw, const void* w_f16,
                         int ldw, const float* bias, const float* w2, float b2, int metric, float max_depth,
                         const void* hpe_f16, int hpe_pix, float* out_f32, void* stream);
/* mde_op_conv_transpose into a channel slot of a wider NHWC map (the DPT / Depth Pro concat buffers):
 * ldo = channels of that map (>= cout), out_f16 = its base + the slot's first channel.  cout % 8 ==
 * 0, ldo % 8 == 0 and out_f16 16-B aligned (every store is 16 B). */
int mde_op_conv_transpose_ld(const void* in_f16, int batch, int h, int w, int cin, const void* w_f16, int ldw,
                             int cout, int stride, const float* bias, void* out_f16, int ldo, void* stream);
/* mde_op_linear_residual (x32) / mde_op_linear_residual_f16 (xh_f16, optional ln_partials) -- exactly
 * one of x32 and xh_f16 -- with the K loop cut into slices when splitk > 1 (small grids with a long
 * K: the batch-1 fc2).  ws holds the slices' fp32 partial sums: the route on 128 x 128 tiles takes 4
 * slices whatever splitk says, so ws must hold max(splitk, 4) * m * n floats.  splitk <= 1: unsplit. */
int mde_op_linear_residual_split(const void* a_f16, int lda, const void* w_f16, int ldw, int m, int n, int k,
                                 const float* bias, const float* layer_scale, float* x32, void* xh_f16, int ldx,
                                 float* ln_partials, int splitk, float* ws, size_t ws_floats, int* tile_cnt,
                                 int tile_cnt_cap, size_t slot_floats, void* stream);
/* ---- since ABI 12: the row, head and patch-embed kernels that only the engine graphs reached, one thin
 * test surface each (no reference counterpart; tests/test_gpu_rows.py, tests/test_gpu_engine_rows.py).
 * No policy of their own. */
/* mde_op_layernorm with fp32 output rows (the exact-fp32 engines' norm1 / norm2 and, with tokens and
 * skip_cls, the taps' final norm: the cls row of every tokens-row sequence dropped, rows % tokens == 0). */
int mde_op_layernorm32(const float* x, float* y, const float* gamma, const float* beta, int rows, int dim, float eps,
                       int tokens, int skip_cls, void* stream);
/* LayerNorm in place over rows [row0, tokens) of every sequence of x [nseq][tokens][dim]; rows [0, row0)
 * are not touched (VGGT: DINOv2's final norm over the patch tokens).  dim: 128, 256, 384, 512, 768, 1024. */
int mde_op_rows_layernorm(float* x, const float* gamma, const float* beta, int nseq, int tokens, int row0, int dim,
                          float eps, void* stream);
/* Rows [0, npre) of every sequence of x [nseq][tokens][dim] = pre [sets][npre][dim]: set 0 (sets == 1), or
 * set 0 for sequence s with s % frames == 0 and set 1 for the others (sets == 2; VGGT's camera / register
 * tokens).  dim % 4 == 0, x and pre 16-B aligned. */
int mde_op_prefix_rows(float* x, const float* pre, int nseq, int tokens, int npre, int dim, int frames, int sets,
                       void* stream);
/* Row 0 of every sequence of x [nseq][tokens][dim] = cls [dim] (Depth Pro's cls + pos[0]). */
int mde_op_cls_rows(float* x, const float* cls, int nseq, int tokens, int dim, void* stream);
/* out[b] = bias + sum_k in[b][k] * w[k], fp32 accumulation (Depth Pro's fov head: the last conv over the
 * whole map as a dot product). */
int mde_op_fov_final(const void* in_f16, const float* w, float bias, int k, int batch, float* out, void* stream);
/* out[m] = act(b2 + sum_c hid[m][c] * w2[c]) over fp32 hid [m][32] (16-B aligned): metric 0 ReLU, 1
 * max_depth * sigmoid, 2 exp (the exact-fp32 head's last 1x1 conv; exp through the hardware's exp2). */
int mde_op_head32(const float* hid, const float* w2, float b2, int m, int metric, float max_depth, float* out,
                  void* stream);
/* mde_op_patch_embed in the engines' form: the image's (h / 14) x (w / 14) whole patches (a remainder of
 * rows / columns is cropped) to rows [tok0, tok0 + patches) of every tokens-row sequence of the fp32
 * stream x32 or the f16 stream xh_f16 (exactly one of them).  cls_pos (optional, tok0 >= 1) -> row 0 of
 * every sequence; without it rows [0, tok0) are not touched (a form of this test surface alone: the
 * engines always pass a cls row, VGGT overwriting it with mde_op_prefix_rows' kernel).  With xh_f16: ln_partials (optional, dim % 32
 * == 0) = fp32 [dim/32][batch*tokens][2], the folded-LayerNorm partials of the patch rows written, and of
 * the cls rows copied from cls_st [dim/32][2]. */
int mde_op_patch_embed_stream(const float* img, int batch, int h, int w, const void* w_f16, int ldw,
                              const float* bias, const float* pos_patch, const float* cls_pos, int dim, int tokens,
                              int tok0, void* patch_scratch_f16, float* x32, void* xh_f16, float* ln_partials,
                              const float* cls_st, void* stream);
/* The exact-fp32 engines' patch embed: fp32 patch rows [batch*patches][672] into patch_scratch_f32, fp32
 * weights [dim_pad][ldw] (mde_op_linear32's layout), x32 [batch][patches + 1][dim]. */
int mde_op_patch_embed32(const float* img, int batch, int h, int w, const float* w_f32, int ldw, const float* bias,
                         const float* pos_patch, const float* cls_pos, int dim, float* patch_scratch_f32, float* x32,
                         void* stream);
/* uint8 NHWC image [batch][h][w][3] -> the patch-embed operand [batch*(h/14)*(w/14)][672] f16
 * (patch-major, channel, row, 16-wide padded column), computing ((float)u / scale - mean[c]) / std[c]
 * in fp32 (the ONNX preamble of reference core/onnx_tools.py:175-199: Cast, Div, Sub, Div). */
int mde_op_patch_prep_u8(const unsigned char* img_u8, int batch, int h, int w, float scale, const float* mean3,
                         const float* std3, void* patches_f16, void* stream);
/* Post-process (reference models/depth_anything_v2/onnx2trt.py:111-117): bilinear
 * align_corners=True resize of fp32 depth [batch][ih][iw] to [batch][oh][ow], then clamp to [lo, hi]. */
int mde_op_depth_postprocess(const float* depth, int batch, int ih, int iw, float* out, int oh, int ow, float lo,
                             float hi, void* stream);
/* Pre-process (since ABI 9; reference core/preprocess.py:preprocess_for for the stretch + imagenet
 * models: cvtColor(BGR2RGB), cv2.resize(INTER_LINEAR) on uint8, /255, standardise, NCHW float32).
 * A restatement of OpenCV's published fixed-point INTER_LINEAR for 8-bit, 3-channel images; parity
 * with cv2 itself is not pinned in this repository, the kernel is pinned bit for bit to
 * monocular_depth_estimation_trt_amd/preprocess.py:resize_linear_u8.  The contract:
 *   per axis (dst outputs from src inputs)
 *     scale = 1.0 / ((double)dst / (double)src)        float64; NOT src / dst
 *     f     = (float)((d + 0.5) * scale - 0.5)         float64, rounded once to float32
 *     s     = floor(f);  f -= s                        float32
 *   horizontal axis only
 *     s <  0         -> s = 0,         f = 0
 *     s >= src_w - 1 -> s = src_w - 1, f = 0
 *     second tap     = min(s + 1, src_w - 1)
 *   vertical axis
 *     f is not changed at the borders; both tap rows s and s + 1 are clamped to [0, src_h - 1]
 *   coefficients, per axis (two separately rounded float32 products, half to even; they need not
 *   sum to 2048)
 *     c0 = rint((1.f - f) * 2048.f),  c1 = rint(f * 2048.f)
 *   horizontal pass, exact integers
 *     H = S[s] * a0 + S[s1] * a1
 *   vertical pass
 *     out = (((b0 * (H0 >> 4)) >> 16) + ((b1 * (H1 >> 4)) >> 16) + 2) >> 2      (always 0..255)
 *   special case: sw == 2 ow AND sh == 2 oh takes cv2's area path, out = (s00 + s01 + s10 + s11 + 2)
 *     >> 2 over the 2x2 block (a 2x ratio on one axis only stays on the linear path).
 * src is [batch][sh][pitch] bytes, 3 interleaved channels per pixel, pitch >= 3 * sw (ROI / aligned
 * rows; bytes of a row past 3 * sw are never read); swap_rb != 0 writes source channel 2 - c to
 * output channel c (BGR -> RGB; commutes with the resize, which is per channel).
 * mde_op_resize_u8 writes uint8 NHWC [batch][oh][ow][3] (the "image_u8" binding of a uint8_nhwc
 * engine); mde_op_resize_u8_norm writes float32 NCHW [batch][3][oh][ow] = lut3x256[c][value] (the
 * "input" binding of a float engine), lut3x256 a device float[3][256] indexed by output channel and
 * resized pixel value (preprocess.py:normalize_lut builds it in the reference's own dtypes).
 * Both only enqueue one kernel on `stream` (no allocation, no synchronisation: capturable).
 * MDE_ERR_ARG, before any device call: null pointer, non-positive size, pitch < 3 * sw. */
int mde_op_resize_u8(const unsigned char* src, int batch, int sh, int sw, int pitch, int swap_rb,
                     unsigned char* dst_u8, int oh, int ow, void* stream);
int mde_op_resize_u8_norm(const unsigned char* src, int batch, int sh, int sw, int pitch, int swap_rb,
                          const float* lut3x256, float* dst_f32_nchw, int oh, int ow, void* stream);
/* Depth Pro photo path (since ABI 10): the two ends of reference models/depth_pro/onnx2trt.py around
 * the engine.  mde_op_dp_preprocess restates :56-74, ToTensor + Normalize(0.5, 0.5) +
 * F.interpolate(bilinear, align_corners=False): src is a uint8 photo [batch][sh][pitch], 3 interleaved
 * channels per pixel, with the rules of mde_op_resize_u8 (pitch >= 3 * sw, bytes of a row past 3 * sw
 * are never read, swap_rb != 0 writes source channel 2 - c to output channel c); dst is float32 NCHW
 * [batch][3][oh][ow], the engine's "input" binding.  The contract:
 *   value of a pixel byte u:  lut[u], a device float[256] the caller passes
 *                             (host builds it as ((float32(u) / 255f) - 0.5f) / 0.5f, all float32)
 *   per axis (dst outputs from src inputs), every operation rounded to float32 separately, never fused:
 *     scale = (float)src / (float)dst
 *     x  = scale * ((float)d + 0.5f) - 0.5f;   x = max(x, 0)
 *     i0 = min((int)x, src - 1);  i1 = min(i0 + 1, src - 1)
 *     l1 = clamp(x - (float)i0, 0, 1);  l0 = 1 - l1
 *   out = b0 * (a0 * v00 + a1 * v01) + b1 * (a0 * v10 + a1 * v11)     (a: horizontal, b: vertical)
 * mde_op_dp_postprocess restates :118-134: inv is "canonical_inverse_depth", fp32 [batch][ih][iw];
 * depth is metric depth, fp32 [batch][oh][ow].  fov_deg is a device float[batch] (the engine's second
 * output binding) and may be null; f_px is a host float, used for every image when fov_deg is null (the
 * reference's f_px0 / EXIF path) and then > 0; f_px_out is a device float[batch], may be null, and
 * receives the focal length actually used.  The contract:
 *   f  = fov_deg ? (0.5f * ow) / tanf(0.5f * (fov_deg[b] * (pi/180))) : f_px
 *   k  = (float)ow / f
 *   tap value = inv * k                 (rounded, before blending - the reference scales, then resizes)
 *   m  = the same bilinear as above, [ih][iw] -> [oh][ow]
 *   depth = 1.0f / min(max(m, 1e-4f), 1e4f)        (IEEE division; the build has no fast-math, keep it so)
 *   a NaN m stays NaN, as in torch.clamp: a non-finite engine output is not turned into a finite depth
 * The kernels are pinned bit for bit to monocular_depth_estimation_trt_amd/preprocess.py:
 * resize_bilinear_f32 and postprocess.py:depth_pro_postprocess_np (except tanf, the device's own), and
 * those to torch on the CPU within a derived tolerance ("Depth Pro photo path").
 * Both only enqueue one kernel on `stream` (no allocation, no synchronisation: capturable).
 * MDE_ERR_ARG, before any device call: a null required pointer, a non-positive size, pitch < 3 * sw,
 * a source or destination plane of 2^31 - 256 elements or more, batch > 65535, post-process with null
 * fov_deg and f_px <= 0. */
int mde_op_dp_preprocess(const unsigned char* src, int batch, int sh, int sw, int pitch, int swap_rb,
                         const float* lut256, float* dst_f32_nchw, int oh, int ow, void* stream);
int mde_op_dp_postprocess(const float* inv, int batch, int ih, int iw, const float* fov_deg, float f_px,
                          float* f_px_out, float* depth, int oh, int ow, void* stream);
/* Point clouds (added to ABI 11 without a new version number -- purely additive; a caller that must
 * know looks the symbol up):
 * the tail of reference models/depth_pro/onnx2trt_pointcloud.py (:172-184),
 * pinhole unprojection of metric depth into PLY binary_little_endian vertex records, on the device.
 * depth is fp32 [batch][h][w] (the output of mde_op_dp_postprocess / mde_op_depth_postprocess); photo is
 * optional, uint8 [batch][h][pitch] of the same h, w, 3 interleaved channels per pixel with the rules of
 * mde_op_resize_u8 (pitch >= 3 * w, bytes of a row past 3 * w are never read, swap_rb != 0 writes source
 * channel 2 - c to output channel c).  f_px_dev is a device float[batch] (the f_px_out of
 * mde_op_dp_postprocess: no host round trip) and may be null; then the host floats fx, fy (> 0) hold for
 * every image.  cx, cy are host floats (the reference uses w / 2, h / 2).  The contract:
 *   sampled grid: hs = ceil(h / step) by ws = ceil(w / step), sample (i, j) is pixel
 *                 (v, u) = (i * step, j * step), z = depth[b][v][u]
 *   fx = fy = f_px_dev[b] when f_px_dev is given, else the host floats fx, fy
 *   every operation float32 and rounded separately, never fused:
 *     xn = ((float)u - cx) / fx          yn = ((float)v - cy) / fy        (IEEE division)
 *     X = xn * z,  Y = yn * z,  Z = z
 *   colour = photo bytes of pixel (v, u), output order R, G, B after swap_rb
 *   record = float X, Y, Z, then uchar R, G, B when a photo is given: rec = 15 bytes (12 without),
 *            tightly packed; image b's region starts at byte b * hs * ws * rec of `records`, whatever
 *            alignment that and the base pointer have
 *   organized (compact == 0): every sample is written, record index = sample index (row-major), no
 *            range test, a NaN z gives NaN X, Y, Z; counts[b] = hs * ws; one kernel
 *   compact: a sample is kept iff z == z && z >= z_lo && z <= z_hi (bounds inclusive; NaN, and +-inf
 *            outside the range, are dropped); the kept records are dense, in row-major sample order;
 *            counts[b] (device int32[batch]) = number kept; bytes of the region past counts[b] records
 *            are not written; the same bytes on every run.  Three kernels (count per workgroup, scan,
 *            write) that need ws, mde_op_point_cloud_ws_bytes(batch, h, w, step) bytes of device
 *            scratch, 4-byte aligned (0 is returned for sizes the op refuses).
 * The kernels are pinned bit for bit to monocular_depth_estimation_trt_amd/pointcloud.py:unproject_np.
 * mde_op_point_cloud only enqueues on `stream` (no allocation, no synchronisation, no host read of
 * counts: capturable).  MDE_ERR_ARG, before any device call: null depth, records or counts; a
 * non-positive size or step; a photo with pitch < 3 * w; f_px_dev null and fx <= 0 or fy <= 0; NaN cx or
 * cy; h * w or hs * ws of 2^31 - 256 or more; batch > 65535; records_bytes < batch * hs * ws * rec;
 * compact with ws null or ws_bytes too small, or z_lo > z_hi. */
size_t mde_op_point_cloud_ws_bytes(int batch, int h, int w, int step);
int mde_op_point_cloud(const float* depth, int batch, int h, int w, int step, const unsigned char* photo, int pitch,
                       int swap_rb, const float* f_px_dev, float fx, float fy, float cx, float cy, int compact,
                       float z_lo, float z_hi, void* records, size_t records_bytes, int* counts, void* ws,
                       size_t ws_bytes, void* stream);
/* Meshes (added to ABI 11 without a new version number, as the point cloud was): the tail of reference
 * models/metric_anything/demo_pointcloud.py (:142-149) -- drop the depth edges (the flying pixels a bilinear
 * resize leaves at an occlusion boundary), then a triangle mesh over what is left, without unreferenced
 * vertices -- on the device.  The arguments up to z_hi mean exactly what they mean for mde_op_point_cloud:
 * the sampled grid hs x ws, the unprojection, the 12- or 15-byte vertex records, image b's vertex region at
 * byte b * hs * ws * rec of `vertices`.  On the sampled grid, all float32:
 *   valid(i, j) = z == z && z >= z_lo && z <= z_hi
 *   edge        zmax and zmin over the valid samples of the 3 x 3 neighbourhood of (i, j) clipped to the grid,
 *               diff = zmax - zmin (one subtraction);
 *               edge = valid && ((edge_atol > 0 && diff > edge_atol) || (edge_rtol > 0 && diff / z > edge_rtol)),
 *               IEEE division, strict comparisons (a sample exactly at the threshold is not an edge); both
 *               tolerances 0: nothing is an edge
 *   clean       valid && !edge
 *   quads       (i, j) for i < hs - 1, j < ws - 1, corners a = (i, j), b = (i, j + 1), c = (i + 1, j + 1),
 *               d = (i + 1, j); kept iff all four corners are clean
 *   diagonal    fabsf(za - zc) <= fabsf(zb - zd): triangles (a, d, c) and (a, c, b); else (a, d, b) and
 *               (b, d, c).  In the camera frame (X right, Y down, Z forward) every triangle faces the origin
 *   vertices    faces != 0: a sample is a vertex iff at least one of its up to four quads is kept; faces == 0:
 *               iff it is clean (the flying-pixel filter for a plain cloud; face_records and face_counts may
 *               then be null).  Records dense, in row-major sample order; vertex_counts[b] their number
 *   faces       record = uchar 3, int32 i0, i1, i2: 13 bytes, tightly packed (a PLY `property list uchar int
 *               vertex_indices` entry), indices into image b's own vertex list; dense, in row-major quad order, a
 *               quad's two triangles adjacent in the order above; image b's region starts at byte
 *               b * 2 * (hs - 1) * (ws - 1) * 13 of `face_records`; face_counts[b] = number of triangles
 * The same bytes on every run; no byte of either region past its count is written and none outside the
 * regions; base pointers of any alignment.  hs < 2 or ws < 2 gives zero faces (and, with faces, zero vertices).
 * Six kernels (four without faces) that need ws, mde_op_depth_mesh_ws_bytes(batch, h, w, step) bytes of device
 * scratch, 4-byte aligned (0 is returned for sizes the op refuses): two ints per 1024 samples, and an int32
 * index and a flag byte per sample.  The kernels are pinned byte for byte to
 * monocular_depth_estimation_trt_amd/pointcloud.py:mesh_np.  mde_op_depth_mesh only enqueues on `stream` (no
 * allocation, no synchronisation, no host read of a count: capturable).  MDE_ERR_ARG, before any device call:
 * everything mde_op_point_cloud refuses in compact mode (of vertices, vertex_counts, vertices_bytes); a negative
 * or NaN tolerance; faces != 0 with null face_records or face_counts, faces_bytes < batch * 2 * (hs - 1) *
 * (ws - 1) * 13, or 2 * (hs - 1) * (ws - 1) of 2^31 - 256 or more; ws null, short or not 4-byte aligned. */
size_t mde_op_depth_mesh_ws_bytes(int batch, int h, int w, int step);
int mde_op_depth_mesh(const float* depth, int batch, int h, int w, int step, const unsigned char* photo, int pitch,
                      int swap_rb, const float* f_px_dev, float fx, float fy, float cx, float cy, float z_lo,
                      float z_hi, float edge_rtol, float edge_atol, int faces, void* vertices, size_t vertices_bytes,
                      int* vertex_counts, void* face_records, size_t faces_bytes, int* face_counts, void* ws,
                      size_t ws_bytes, void* stream);
/* Depth evaluation (added to ABI 11 without a new version number, as the point cloud was): the per-image
 * call sequence of reference tools/evaluate_gt.py:555-583 over core/gt.py (orientation, align, metrics), on
 * the device.  pred and gt are fp32 [batch][h][w] (pred: the output of mde_op_depth_postprocess /
 * mde_op_dp_postprocess; gt in metres), mask is uint8 [batch][h][w], nonzero = measured.  policy: 0 none,
 * 1 scale, 2 scale_shift.  max_depth <= 0: no range limit.  out is a device double[batch][16]:
 *   0 status   0 scored; 1 fewer than two fit pixels; 2 scale_shift underdetermined (constant prediction)
 *   1 n_fit    pixels the fit used (0 under policy none)
 *   2 scale    NaN where nothing was fitted (policy none, status != 0)
 *   3 shift    NaN unless policy scale_shift fitted one
 *   4 n        pixels scored
 *   5 abs_rel  6 rmse  7 log10  8 delta1  9 delta2  10 delta3     (NaN when n == 0)
 *   11 orientation (Pearson correlation of pred and gt; NaN when undefined)
 *   12 n_mask  pixels of m below (what separates the reference's two "fewer than two pixels" messages)
 *   13..15 written as 0
 * Per image, every per-pixel operation in float64 with one rounding per operation (x * s + t rounds twice):
 *   m = mask && gt > 0
 *   orientation: over m && isfinite(pred), from n, Sa, Sb, Saa, Sbb, Sab (a = pred, b = gt):
 *     saa = Saa - Sa * Sa / n, sbb and sab likewise, sab / sqrt(saa * sbb); NaN when n < 2 or saa <= 0 or sbb <= 0
 *   fit, scale: over m (narrowed to finite pred when fit_finite_only), s = Spg / max(Spp, 1e-12) where a
 *     NaN Spp stays NaN; aligned = pred * s.  Without fit_finite_only one non-finite pred under m makes s NaN.
 *   fit, scale_shift: over m && isfinite(pred), and pred > 0 unless pred_is_inverse; x = pred if inverse else
 *     1 / pred, y = 1 / gt; d = n * Sxx - Sx * Sx, s = (n * Sxy - Sx * Sy) / d, t = (Sy - s * Sx) / n;
 *     over the whole frame disp = x * s + t (x = NaN for pred <= 0 when not inverse),
 *     aligned = disp > 1e-8 ? 1 / disp : +inf
 *   fit, none: aligned = pred
 *   status 1 when n_fit < 2, status 2 when |d| < 1e-12; then n = 0 and slots 5..10 are NaN
 *   metrics: over m && isfinite(aligned), and gt <= max_depth when a limit is given; p = max(aligned, 1e-6),
 *     ratio = max(p / g, g / p); n, mean |p - g| / g, sqrt(mean (p - g)^2), mean |log10 p - log10 g|, and
 *     the fractions ratio < 1.25, < 1.5625, < 1.953125
 * Four kernels.  A workgroup owns MDE_DEPTH_EVAL_TILE consecutive pixels of one image, whatever the grid
 * or the card, and writes that tile's partial sums to ws; one workgroup per image adds them in a fixed
 * order.  No workgroup waits on another's writes and there are no floating-point atomics: the same 128
 * bytes per image on every run.  ws: mde_op_depth_eval_ws_bytes(batch, h, w) bytes of device scratch,
 * 8-byte aligned (0 is returned for sizes the op refuses).  The kernels are held to
 * monocular_depth_estimation_trt_amd/evaluate.py:score_np within the summation-order tolerance derived in
 * DESIGN.md, "Scoring against ground truth".  mde_op_depth_eval only enqueues on `stream` (no allocation,
 * no synchronisation, no host read: capturable).  MDE_ERR_ARG, before any device call: a null pointer; a
 * non-positive size; a policy outside 0..2; h * w of 2^31 - 256 or more; batch > 65535; NaN max_depth; ws
 * null or ws_bytes too small; out or ws not 8-byte aligned. */
#define MDE_DEPTH_EVAL_TILE 1024
size_t mde_op_depth_eval_ws_bytes(int batch, int h, int w);
int mde_op_depth_eval(const float* pred, const float* gt, const unsigned char* mask, int batch, int h, int w,
                      int policy, int pred_is_inverse, int fit_finite_only, float max_depth, double* out, void* ws,
                      size_t ws_bytes, void* stream);
/* Colour frames (added to ABI 11 without a new version number, as the point cloud and the evaluation were):
 * the closing lines of the reference drivers (models/depth_pro/onnx2trt.py:156-168,
 * models/depth_anything_v2/onnx2trt.py:131-150, models/vggt/onnx2trt.py:122-142) and core/viz.py:colorize,
 * on the device.  map is fp32 [batch][h][w] (the output of mde_op_depth_postprocess / mde_op_dp_postprocess),
 * out_u8 is uint8 [batch][h][w][3], tightly packed.  lut257x3 is a device uchar[257][3] in R, G, B order:
 * entries 0..255 are the colour map, entry 256 the colour of a pixel that has no index ("bad").
 * swap_rb != 0 writes B, G, R (the reference's cvtColor(RGB2BGR)).  range_out may be null; otherwise a
 * device float[batch][2] that receives the range actually used.  Each image is ranged on its own.  Every
 * float operation is float32 and rounded separately, division is IEEE; mode 2 is float64.
 *   mode 0, inverse_auto (the metric drivers: inverse depth clipped to [1/250, 10] for display):
 *     v   = map_is_inverse ? x : 1.0f / x
 *     vmn, vmx = min, max of v over the pixels whose v is finite
 *     c   = (float)(1.0 / 250)
 *     lo  = vmn > c ? vmn : c          hi = vmx < 10.0f ? vmx : 10.0f
 *     d   = (vmx > 10.0f && vmn <= c) ? (float)(10.0 - 1.0 / 250 + denom_eps)    sum in double, one rounding
 *                                     : (hi - lo) + (float)denom_eps             float32
 *     n   = (v - lo) / d;  t = n * 256.0f
 *     index: NaN t -> 256 (bad); t < 0 -> 0; t >= 256 -> 255; else (int)t
 *     range_out = {lo, hi}
 *     (the two-way d is the reference's arithmetic under NumPy's promotion rules: Python's min / max return
 *     Python floats when both ends clip, so that one difference is taken in double; denom_eps = 1e-6 is
 *     the VGGT driver's variant)
 *   mode 1, minmax_u8 (the relative driver):
 *     mn, mx over finite x;  q = ((x - mn) / (mx - mn)) * 255.0f
 *     index: NaN q -> 256; q < 0 (-inf) -> 0; q >= 255 (+inf) -> 255; else (int)q
 *     range_out = {mn, mx}
 *   modes 0 and 1 without one finite value: range_out = {NaN, NaN} and every pixel is bad; a constant map
 *     (with denom_eps == 0) gives 0 / 0 and is bad, as matplotlib draws it
 *   mode 2, fixed (core/viz.py:colorize, a caller-given axis, "never on its own range"), in float64:
 *     vmax <= vmin -> vmax = vmin + 1e-6
 *     t = clamp(((double)x - vmin) / (vmax - vmin), 0, 1);  index = min((int)(t * 256), 255)
 *     non-finite x (or a NaN t, from an infinite bound) -> 256
 *     range_out = {(float)vmin, (float)vmax};  map_is_inverse and denom_eps are ignored
 * Modes 0 and 1 take three kernels: a workgroup owns MDE_DEPTH_COLORIZE_TILE consecutive pixels of one image
 * and writes that tile's min and max to ws, one workgroup per image finishes lo, hi and d, and the colour
 * pass looks the table up; mode 2 is the colour pass alone.  Pixels before the first and after the last
 * 16-byte aligned group of 16 take one more, scalar launch.  No workgroup waits on another's writes and
 * there are no floating-point atomics: the same bytes on every run.  Bytes past batch * h * w * 3 of out_u8
 * are not written.  ws: mde_op_depth_colorize_ws_bytes(batch, h, w) bytes of device scratch, 4-byte aligned
 * (0 is returned for sizes the op refuses); mode 2 reads none.  The kernels are pinned byte for byte to
 * monocular_depth_estimation_trt_amd/visualize.py:colorize_np.  mde_op_depth_colorize only enqueues on
 * `stream` (no allocation, no synchronisation, no host read: capturable).  MDE_ERR_ARG, before any device
 * call: a null map, out_u8 or lut257x3; a non-positive size; a mode outside 0..2; NaN denom_eps; mode 2
 * with a NaN bound; h * w of 2^31 - 256 or more; batch > 65535; in modes 0 and 1 ws null, ws_bytes too
 * small or ws not 4-byte aligned; range_out not 4-byte aligned. */
#define MDE_DEPTH_COLORIZE_TILE 4096
size_t mde_op_depth_colorize_ws_bytes(int batch, int h, int w);
int mde_op_depth_colorize(const float* map, int batch, int h, int w, int mode, int map_is_inverse, double denom_eps,
                          double vmin, double vmax, const unsigned char* lut257x3, int swap_rb,
                          unsigned char* out_u8, float* range_out, void* ws, size_t ws_bytes, void* stream);
/* Robust display range (added to ABI 11 without a new version number, as the four additions before it): the
 * reference's core/viz.py:robust_range / display_ranges / qualitative_display and demo.py:distribution, on
 * the device -- exact percentiles of the valid pixels of fp32 maps [batch][h][w], as np.percentile (method
 * linear, numpy 2.2) computes them in float64.  out is a device double[rows][8], rows = 1 when pooled, else
 * batch.  q_percent is a HOST array of nq (1..3) percentages, read before the call returns.
 *   valid pixel   finite, and > 0 when positive_only; -0 counts as +0
 *   order         a valid pixel's rank r is its position among the valid pixels of its image, row-major
 *   subsample     (the reference's v[:: max(1, v.size // 200000)]) stride = max(1, n_valid / sample_cap) in
 *                 integer division when sample_cap > 0 and n_valid > sample_cap, else 1; a valid pixel is used
 *                 iff r % stride == 0.  sample_cap = 200000 is the reference's, 0 takes every valid pixel
 *   sample        per image: the used values widened to float64; pooled: every image's used values together,
 *                 each image with its own stride; reciprocal: 1.0 / x in float64 of each (1 / 0 = +inf)
 *   quantile p of the n sorted sample values s, every operation float64 and rounded separately:
 *                 q = p / 100; vi = (n - 1) * q; prev = floor(vi), next = prev + 1, both n - 1 when vi >= n - 1;
 *                 g = vi - floor(vi); d = s[next] - s[prev]; g < 0.5 ? s[prev] + d * g : s[next] - d * (1 - g)
 *   out[row][.]   0 n_valid   1 n_used (the sample's size)   2 min of the sample   3 max of the sample
 *                 4 quantile 0   5 quantile 1 (0 when nq == 1)   6, 7 the display range {vmin, vmax}
 *                 nq == 3: slot 3 holds quantile 2 instead of the max -- eight slots cannot hold nine values,
 *                 and slots 6, 7 are what mde_op_depth_colorize_ranged reads; the max still enters the range
 *   display range vmin = quantile 0, vmax = quantile nq - 1; if either is not finite or vmax <= vmin: {min,
 *                 max} of the sample, and if still vmax <= vmin: vmax = vmin + 1.0
 *   empty sample  slots 2..5 NaN, display range {0.0, 1.0}
 * Selection is a radix select over four 8-bit digits of an order-preserving 32-bit key (the float's bits,
 * sign-flipped; under reciprocal a key ordered as 1 / x is), so it is exact: a workgroup owns
 * MDE_DEPTH_QUANTILES_TILE consecutive pixels of one image, counts digits in LDS and adds them to ws with
 * integer atomics, whose sums do not depend on the order; there are no floating-point atomics, and the same
 * 64 bytes per row come out on every run.  ws: mde_op_depth_quantiles_ws_bytes(batch, h, w) bytes of device
 * scratch, 8-byte aligned (0 is returned for sizes the op refuses; enough for pooled or not); its content on
 * entry does not matter, the op zeroes what it counts in on `stream`.  The kernels are pinned bit for bit to
 * monocular_depth_estimation_trt_amd/visualize.py:quantiles_np.  mde_op_depth_quantiles only enqueues on
 * `stream` (no allocation, no synchronisation, no host read of device memory: capturable).  MDE_ERR_ARG,
 * before any device call: a null pointer; a non-positive size; nq outside 1..3; a q_percent outside [0, 100]
 * or NaN; a negative sample_cap; h * w of 2^31 - 256 or more; batch > 65535; pooled with batch * h * w of
 * 2^31 - 256 or more; ws null, ws_bytes too small; out or ws not 8-byte aligned.
 * mde_op_depth_colorize_ranged is mode 2 of mde_op_depth_colorize with the axis read from device memory:
 * image b is drawn on vmin = range_dev[b * range_stride], vmax = range_dev[b * range_stride + 1] (stride 0:
 * one shared axis; out + 6 of the quantile op with stride 8: its rows).  A pixel is valid when it is finite,
 * and > 0 when positive_only; y = reciprocal ? 1.0 / (double)x : (double)x; then mode 2's lines on y
 * (vmax <= vmin -> vmax = vmin + 1e-6, clamp, min((int)(t * 256), 255)); an invalid pixel or a NaN t gets
 * index 256.  With both flags 0 and the same bounds the picture is mode 2's, byte for byte.  Enqueue only.
 * MDE_ERR_ARG, before any device call: a null pointer; a non-positive size; a negative range_stride;
 * range_dev not 8-byte aligned; h * w of 2^31 - 256 or more; batch > 65535. */
#define MDE_DEPTH_QUANTILES_TILE 4096
size_t mde_op_depth_quantiles_ws_bytes(int batch, int h, int w);
int mde_op_depth_quantiles(const float* map, int batch, int h, int w, int positive_only, int reciprocal, int pooled,
                           int sample_cap, const double* q_percent, int nq, double* out, void* ws, size_t ws_bytes,
                           void* stream);
int mde_op_depth_colorize_ranged(const float* map, int batch, int h, int w, int positive_only, int reciprocal,
                                 const double* range_dev, int range_stride, const unsigned char* lut257x3,
                                 int swap_rb, unsigned char* out_u8, void* stream);
/* Point-cloud preview (added to ABI 11 without a new version number, as the additions before it): the
 * reference's core/viz.py:render_points, what demo.py:cloud_figure shows of a cloud -- an orthographic,
 * z-buffered picture of the point cloud "viewed from above-left", centred on the per-axis median, scaled by
 * the 99th percentile of the rotated |x|, |y|, the near point winning each pixel -- on the device, from the
 * depth map, without the records or the float map leaving it.  depth, batch, h, w, step, photo, pitch,
 * swap_rb, f_px_dev, fx, fy, cx, cy mean exactly what they mean for mde_op_point_cloud.  cos_a, sin_a, cos_e,
 * sin_e are HOST doubles: the caller's np.cos / np.sin of the azimuth and the elevation in radians (the
 * reference's defaults: elev -18, azim 24 degrees).  bg_rgb is a HOST int[3], 0..255, in R, G, B order (the
 * reference's 22, 22, 26).  out_u8 is uint8 [batch][out_h][out_w][3], tightly packed; out_swap_rb != 0 writes
 * B, G, R.  view_out is a device double[batch][8]; view_in is null or a device double[batch][8].  The contract,
 * every operation rounded separately, never fused:
 *   points      sample i of the hs x ws step grid has X, Y, Z as in mde_op_point_cloud (float32, organized
 *               order); it is valid iff X, Y and Z are finite and Z > 0 (the reference's subsample_cloud).
 *               Every valid sample is drawn: the reference's random thinning to 120000 points is NOT
 *               reproduced, so parity with it is claimed for clouds up to that size (`step` gets a larger map
 *               there)
 *   centre      c[k] = percentile 50 of the valid X, Y, Z values respectively, as mde_op_depth_quantiles
 *               computes a quantile (-0 counts as +0, float64 lerp).  np.median takes the mean of the two
 *               middle values at an even count, (a + b) / 2; the lerp gives a + (b - a) * 0.5 (or its mirror),
 *               which differs from it by at most one float64 rounding; at an odd count they are equal
 *   rotation    float64, from the doubles of X, Y, Z:
 *                 dx = X - c0, dy = Y - c1, dz = Z - c2
 *                 x1 = cos_a * dx + sin_a * dz          z1 = (-sin_a) * dx + cos_a * dz
 *                 y2 = cos_e * dy - sin_e * z1          z2 = sin_e * dy + cos_e * z1
 *   span        percentile 99 of the 2 * n_valid float32 values (float)|x1|, (float)|y2| pooled, by the same
 *               quantile arithmetic; 1.0 when that is not finite or <= 0
 *   scale       (0.46 * min(out_h, out_w)) / span
 *   pixel       u = rint(x1 * scale + out_w / 2.0), v = rint(y2 * scale + out_h / 2.0), half to even, float64;
 *               inside iff 0 <= u < out_w and 0 <= v < out_h, tested on the doubles (a NaN is outside)
 *   winner      of a pixel: among the valid samples inside it the smallest (float)z2, compared as floats with
 *               -0 equal to +0 (the reference compares the doubles: a float32 z-test key is this op's); among
 *               equal ones the lowest sample index.  Its colour is the photo's bytes of that sample, R, G, B
 *               after swap_rb, or (200, 200, 200) without a photo.  A pixel with no sample gets bg_rgb
 *   view_out[b] {n_valid, c0, c1, c2, span, scale, samples inside the picture, 0}; with no valid sample:
 *               centre 0, span 1.0, nothing drawn
 *   view_in     non-null: image b takes c0, c1, c2 and scale from view_in[b] (slots 1, 2, 3, 5), no selection
 *               runs, and view_out[b] repeats slots 1..5 of view_in[b] with its own two counts -- the fixed
 *               camera for a frame sequence.  view_in may be view_out
 * Only the reference's default point_px = 1 is built (for larger values it lets later offsets paint over
 * nearer points).  Without view_in the op writes X, Y, Z as three float32 planes (NaN where invalid) and
 * selects the three medians with the kernels of mde_op_depth_quantiles, overwrites two planes with |x1|, |y2|
 * and selects the span with one pooled call per image; then, in both cases, it clears a z-buffer
 * uint64[batch][out_h * out_w] to all ones, every valid sample inside the picture does one 64-bit integer
 * atomic min of (order-preserving key of (float)z2) << 32 | sample index, and one thread per pixel writes
 * the winner's three bytes.  The only atomic is that integer min (the two counts are summed from per-workgroup
 * slots), no workgroup waits on another's writes: the same bytes on every run.  Bytes past batch * out_h * out_w * 3 of out_u8 are not written.
 * ws: mde_op_cloud_view_ws_bytes(...) bytes of device scratch (planes, z-buffer, quantile rows and
 * scratch), 8-byte aligned (0 is returned for sizes the op refuses); its content on entry does not matter.
 * The kernels are pinned to monocular_depth_estimation_trt_amd/pointcloud.py:render_np, the picture byte for
 * byte and the view rows bit for bit; render_np against the reference's render_points: DESIGN.md,
 * "Point-cloud preview".  mde_op_cloud_view only enqueues on `stream` (no allocation, no synchronisation, no
 * host read of device memory: capturable).  MDE_ERR_ARG, before any device call: null depth, out_u8,
 * view_out or bg_rgb; a non-positive size or step; a photo with pitch < 3 * w; f_px_dev null and fx <= 0 or
 * fy <= 0; NaN cx or cy; h * w of 2^31 - 256 or more; hs * ws of 2^30 - 128 or more (two planes are pooled in
 * one selection); batch > 21845 (three planes per image); a non-positive picture size or out_h * out_w of
 * 2^31 - 256 or more; a NaN or infinite trig value; a background colour outside 0..255; ws null, ws_bytes too
 * small; ws, view_in or view_out not 8-byte aligned. */
size_t mde_op_cloud_view_ws_bytes(int batch, int h, int w, int step, int out_h, int out_w);
int mde_op_cloud_view(const float* depth, int batch, int h, int w, int step, const unsigned char* photo, int pitch,
                      int swap_rb, const float* f_px_dev, float fx, float fy, float cx, float cy, double cos_a,
                      double sin_a, double cos_e, double sin_e, const double* view_in, const int* bg_rgb,
                      int out_swap_rb, unsigned char* out_u8, int out_h, int out_w, double* view_out, void* ws,
                      size_t ws_bytes, void* stream);
/* VGGT photo path (added to ABI 11 without a new version number, as the three additions before it): the two
 * ends of reference models/vggt/onnx2trt.py (:32-53, :121-146) around the engine, over core/preprocess.py:
 * resize_square_pad -- cvtColor(BGR2RGB), copyMakeBorder(BORDER_CONSTANT, white) to a square, one
 * cv2.resize(INTER_CUBIC) on uint8, /255 in float32 -- and the crop of the depth map to the content box.
 * mde_op_resize_cubic_u8 is a restatement of OpenCV's published scalar fixed-point INTER_CUBIC for 8-bit,
 * 3-channel images; parity with cv2 itself is not pinned in this repository ("VGGT photo path"),
 * the kernel is pinned bit for bit to monocular_depth_estimation_trt_amd/preprocess.py:resize_cubic_u8.
 * One more caveat than for the linear resize: vectorised builds of OpenCV evaluate the VERTICAL pass in
 * float32 (beta / 2^22 multiply-adds, then round) instead of the integer form below, and can differ from it
 * by one level on pixels whose exact sum sits at a rounding boundary.  The contract is the scalar integer form:
 *   virtual source: ph = pad_top + sh + pad_bottom rows by pw = pad_left + sw + pad_right columns; pixel
 *     (y, x) of it is the photo's pixel (y - pad_top, x - pad_left) where that lies inside the photo and the
 *     pad colour everywhere else.  No padded copy is made.  All four pads zero: a plain cubic resize.
 *   per axis (dst outputs from src = pw or ph inputs), the same on both axes; unlike the linear kernel no
 *   fraction is zeroed at a border
 *     scale = 1.0 / ((double)dst / (double)src)        float64; NOT src / dst
 *     f     = (float)((d + 0.5) * scale - 0.5)         float64, rounded once to float32
 *     s     = floor(f);  x = f - s                     float32
 *     taps  = s - 1, s, s + 1, s + 2, each clamped to [0, src - 1] of the VIRTUAL image
 *   coefficients, float32, every operation rounded separately in exactly this order, never fused;
 *   A = -0.75f (the constants 5A, 8A, 4A, A + 2, A + 3 are exact)
 *     x1 = x + 1
 *     c0 = ((A*x1 - 5*A)*x1 + 8*A)*x1 - 4*A
 *     c1 = (((A + 2)*x - (A + 3))*x)*x + 1
 *     g  = 1 - x
 *     c2 = (((A + 2)*g - (A + 3))*g)*g + 1
 *     c3 = ((1 - c0) - c1) - c2
 *     k_i = rint(c_i * 2048.f)      half to even; the four need not sum to 2048 (2047..2049 occur)
 *   horizontal pass, exact integers, no shift
 *     H = sum_i S[tap_i] * a_i
 *   vertical pass
 *     V = sum_j H_j * b_j;  out = clamp((V + (1 << 21)) >> 22, 0, 255)         arithmetic shift
 *     (sum |c_i| <= 1.375, reached at x = 0.5, so |V| + 2^21 <= 255 * 2818^2 + 2^21 < 2^31: int32 holds it)
 * src is [batch][sh][pitch] bytes with the rules of mde_op_resize_u8 (3 interleaved channels per pixel,
 * pitch >= 3 * sw, bytes of a row past 3 * sw are never read, swap_rb != 0 writes source channel 2 - c to
 * output channel c).  pad_c0, pad_c1, pad_c2 are the pad colour, host ints 0..255 in OUTPUT channel order
 * (the reference pads after its BGR -> RGB).  mde_op_resize_cubic_u8 writes uint8 NHWC [batch][oh][ow][3];
 * mde_op_resize_cubic_u8_norm writes float32 NCHW [batch][3][oh][ow] = lut3x256[c][value] (the engine's
 * "images" binding [1][S][3][oh][ow] with batch = S), lut3x256 a device float[3][256] indexed by output channel
 * and resized pixel value (preprocess.py:vggt_lut: float32(u) / 255).
 * mde_op_crop_f32 copies the window rows [y0, y0 + ch), columns [x0, x0 + cw) of each fp32 map [batch][h][w]
 * to dst [batch][ch][cw], tightly packed (the reference's depth[round(y1):round(y2), round(x1):round(x2)]).
 * Each of the three only enqueues one kernel on `stream` (no allocation, no synchronisation: capturable);
 * nothing is written outside the destination.  MDE_ERR_ARG, before any device call: a null pointer; a
 * non-positive size; pitch < 3 * sw; a negative pad; a pad colour outside 0..255; a source, virtual or
 * destination plane of 2^31 - 256 elements or more; batch > 65535; a crop window not inside [0, h) x [0, w). */
int mde_op_resize_cubic_u8(const unsigned char* src, int batch, int sh, int sw, int pitch, int swap_rb,
                           int pad_top, int pad_bottom, int pad_left, int pad_right, int pad_c0, int pad_c1,
                           int pad_c2, unsigned char* dst_u8, int oh, int ow, void* stream);
int mde_op_resize_cubic_u8_norm(const unsigned char* src, int batch, int sh, int sw, int pitch, int swap_rb,
                                int pad_top, int pad_bottom, int pad_left, int pad_right, int pad_c0, int pad_c1,
                                int pad_c2, const float* lut3x256, float* dst_f32_nchw, int oh, int ow,
                                void* stream);
int mde_op_crop_f32(const float* src, int batch, int h, int w, int y0, int x0, int ch, int cw, float* dst,
                    void* stream);
/* DA-V2 family native profile (added to ABI 11 without a new version number, as the additions before it):
 * the input half of reference models/depth_anything_ac/onnx2trt.py's `native` profile over core/preprocess.py
 * (preprocess_for(img, model, size, stretch=False)): cvtColor(BGR2RGB), no first resize, /255 in T, ONE
 * cv2.resize(INTER_CUBIC) of the FLOAT image to the keep-ratio size (preprocess.py:native_size), standardise
 * in float64, float32 NCHW -- read straight from the uint8 photo; the float image is never materialised.
 * It restates OpenCV's published SCALAR INTER_CUBIC for CV_32FC3 (wide == 0, T = float: depth_anything_ac)
 * and CV_64FC3 (wide == 1, T = double: depth_anything_v2); parity with cv2 itself is not pinned in this
 * repository ("Native profile": vectorised builds nest the float32 vertical pass as multiply-adds
 * in the opposite order, IPP builds replace the routine; both can differ in the last bit of a float32), the
 * kernel is pinned bit for bit to monocular_depth_estimation_trt_amd/preprocess.py:resize_cubic_float plus
 * the standardise.  The contract:
 *   per axis: scale, f, s, x, the taps s - 1 .. s + 2 clamped to [0, src - 1] and the float32 coefficients
 *   c0 .. c3 exactly as for mde_op_resize_cubic_u8 above (no pad: the virtual image is the photo); the
 *   coefficients stay float32, there is no rint(c * 2048)
 *   sample: S = scale_lut[u], scale_lut a device T[256] the caller filled with (T)u / (T)255
 *   horizontal pass, a_i the column coefficients, each product and each sum rounded once in T, left to right
 *   (a float32 coefficient times a float64 sample is a float64 product), never fused
 *     H = ((S[t0]*a0 + S[t1]*a1) + S[t2]*a2) + S[t3]*a3
 *   vertical pass, b_j the row coefficients, the same discipline; no clamp, cubic overshoot outside [0, 1] stays
 *     V = ((H0*b0 + H1*b1) + H2*b2) + H3*b3
 *   out[c] = (float)(((double)V[c] - mean_c) / std_c)      float64, rounded once to float32
 * src is [batch][sh][pitch] bytes with the rules of mde_op_resize_u8 (3 interleaved channels per pixel,
 * pitch >= 3 * sw, bytes of a row past 3 * sw are never read, swap_rb != 0 writes source channel 2 - c to
 * output channel c); mean0..2 / std0..2 are in OUTPUT channel order; dst is float32 NCHW [batch][3][oh][ow]
 * (the engine's "input" binding).  Only enqueues one kernel on `stream` (no allocation, no synchronisation:
 * capturable); nothing is written outside the destination.  MDE_ERR_ARG, before any device call: a null
 * pointer; a non-positive size; pitch < 3 * sw; wide not 0 or 1; scale_lut not aligned to T or dst not to 4
 * bytes; a NaN mean; a zero or NaN std; a source or destination plane of 2^31 - 256 elements or more;
 * batch > 65535. */
int mde_op_resize_cubic_f_norm(const unsigned char* src, int batch, int sh, int sw, int pitch, int swap_rb,
                               int wide,                       /* 0: T = float, 1: T = double */
                               const void* scale_lut,          /* device T[256]: (T)u / (T)255, made on the host */
                               double mean0, double mean1, double mean2,   /* output channel order */
                               double std0, double std1, double std2,
                               float* dst, int oh, int ow, void* stream);  /* dst: [batch][3][oh][ow] */
/* Depth Pro pyramid patches (upstream DepthProEncoder._create_pyramid + _split, reference engine input
 * "input"): fp32 NCHW image [batch][3][size][size] (size = 4 * 384) -> f16 patch-embed rows
 * [nseq * batch * 576][768] ((c, py, px) order), sequence s = patch * batch + image with the 25
 * x1 patches (stride 288) first, then the 9 x0.5 patches (stride 192), then the x0.25 image;
 * downsampling = bilinear, align_corners=False, computed on the fly. */
int mde_op_dp_pyramid_patches(const float* img, int batch, int size, void* patches_f16, void* stream);
/* Merge encoder rows x32 [.. sequences][tokens][dim] (row 0 of each sequence = cls, dropped) of
 * the n x n patches (base + r*n + c) * batch + b into an NHWC f16 map [batch][side][side][dim],
 * side = n*g - 2(n-1)*pad, trimming `pad` rows/cols on interior patch edges (upstream _merge);
 * gamma/beta non-null: LayerNorm(eps) fused into the gather, else a plain fp32 -> f16 copy. */
int mde_op_merge_tokens(const float* x32, int batch, int tokens, int dim, int n, int g, int pad, int base,
                        const float* gamma, const float* beta, float eps, void* out_f16, void* stream);
/* VGGT attention prologue (upstream vggt layers/attention.py q_norm / k_norm + layers/rope.py
 * RotaryPositionEmbedding2D, base 100), in place on the head-major rows q/k [bh][tokens_pad][64]
 * f16 (the layout mde_op_qkv writes): LayerNorm(64, eps) with q_gamma/q_beta resp. k_gamma/k_beta,
 * then 2D RoPE -- token t sits at frame position p = t % frame_tokens; p < npre is at RoPE
 * position (0, 0), patch p - npre at (row + 1, col + 1) of a grid grid_w wide; features [0, 32)
 * rotate with the row, [32, 64) with the column (rotate_half inside each half); rope_cos /
 * rope_sin are fp32 [>= max position + 1][16] tables of angle(pos, j) = pos * 100^(-j/16) --
 * and finally q *= q_scale.  Rows >= tokens are not touched. */
int mde_op_qk_norm_rope(void* q_f16, void* k_f16, const float* q_gamma, const float* q_beta, const float* k_gamma,
                        const float* k_beta, int bh, int tokens, int tokens_pad, int frame_tokens, int npre,
                        int grid_w, const float* rope_cos, const float* rope_sin, float q_scale, float eps,
                        void* stream);
/* VGGT depth-head tap (upstream heads/dpt_head.py: self.norm over aggregated_tokens_list[i]
 * [:, :, patch_start_idx:], the list entries being cat(frame_out, global_out)): LayerNorm(2*dim,
 * eps) over cat(xa[row], xb[row]) for the patch rows npre .. tokens-1 of each of nseq sequences
 * (xa, xb fp32 [nseq][tokens][dim]) -> f16 [nseq * (tokens - npre)][2*dim]. */
int mde_op_tap_concat_ln(const float* xa, const float* xb, int nseq, int tokens, int npre, int dim,
                         const float* gamma, const float* beta, float eps, void* out_f16, void* stream);
#ifdef __cplusplus
}
#endif

#endif /* MDE_H_ */
