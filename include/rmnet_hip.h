/*
 * rmnet_hip.h -- C ABI of librmnet_hip.so: RMNet's per-frame hot path on MI355X (gfx950).
 *
 * This is the drop-in boundary.  Every entry point replaces one native
 * interface (or one torch-op sequence) of the reference, hzxie/RMNet; paths below are relative
 * to the reference checkout.  Conventions for all calls:
 *   - plain pointers + sizes; all tensor pointers are DEVICE pointers unless the name ends in
 *     _host; tensors are dense row-major fp32 / int32 in the reference's own layouts;
 *   - the caller owns every buffer (inputs, outputs, workspace); nothing is allocated inside;
 *   - asynchronous on `stream` (a hipStream_t passed as void*; NULL = the default stream);
 *     no host synchronisation, so calls can be captured in a hipGraph;
 *   - return value: RMNET_OK (0) or a negative RMNET_E_* code -- errors are returned, never
 *     printed-and-ignored (the reference prints launch errors and carries on,
 *     extensions/reg_att_map_generator/reg_att_map_generator.cu:117-121);
 *   - re-entrant: no global mutable state, safe from one host thread per GPU
 *     (utils/eval_server.py:249-255 calls the op that way).
 */
#ifndef RMNET_HIP_H_
#define RMNET_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RMNET_ABI_VERSION 6   /* 2: rmnet_bank_read_f32 takes a mutable bank; rmnet_bank_area_offset.  3: RMNET_MR_F16 / RMNET_BANK_F16,
                               * rmnet_bank_read_f32_at takes flags.  4: banks of any Tcap, chunked reads of T > 2048 (rmnet_bank_read_workspace_bytes_for);
                               * the read counts out-of-window query elements; sticky error bits + time-out word behind the overflow word.
                               * 5: RMNET_MR_QX / RMNET_BANK_QX (fp16 operands with an exact query); a pair whose merge timed out is
                               * written as NaN; the overflow word is a zero / non-zero flag, not an element count.
                               * 6: the bank keeps the largest affinity logit its reads have seen (third int32 of the control block); channels-last glue entries */

enum {
  RMNET_OK = 0,
  RMNET_E_INVALID_ARG = -1, /* null pointer, non-positive size, unsupported combination */
  RMNET_E_WORKSPACE = -2,   /* workspace pointer null or too small                        */
  RMNET_E_LAUNCH = -3,      /* hipGetLastError() after a launch / memcpy was not success   */
  RMNET_E_UNSUPPORTED = -4  /* shape outside what the kernels implement (see each call)    */
};

int rmnet_abi_version(void);
const char *rmnet_error_string(int code);

/* ---------------------------------------------------------------------------------------------
 * G1/G2  Regional attention map generator.
 * Replaces: pybind `reg_att_map_generator.forward(mask, prob_threshold, n_pts_threshold,
 *           n_bbox_loose_pixels)` -- extensions/reg_att_map_generator/reg_att_map_generator_cuda.cpp:26-38
 *           and its kernel, reg_att_map_generator.cu:15-123.
 *   mask     [B,K,H,W] f32 (soft masks; channel 0 = background, never inspected)
 *   att_map  [B,K,H,W] f32 out: 1 inside the loosened box of channel k>=1, else 0; channel 0 all 0.
 *            May be NULL: the full-resolution map is then not written (the fused regional read
 *            below only needs the boxes).
 *   bboxes   [B,K,4] int32 out: (x_min, x_max, y_min, y_max); channel 0 = (0,0,0,0).
 *   cell_rects [B,K,4] int32 out, may be NULL: the box expressed on the 1/`cell_stride` feature
 *            grid as (cx0, cx1, cy0, cy1) inclusive -- exactly the cells that survive
 *            F.interpolate(att_map padded by (pad_l, pad_t), scale_factor=1/cell_stride)
 *            (models/rmnet.py:245, 307, 356); empty boxes and channel 0 give (1,0,1,0).
 *            cells_h x cells_w is the feature-grid size.
 * Outputs are fully written (no pre-zeroing needed).  Integer outputs are bit-exact.
 * RMNET_E_INVALID_ARG for a NULL mask / bboxes, a non-positive size, H or W > 32767 (the reference's box search starts
 * from 32767) and cell_rects with a non-positive cell_stride / cells_h / cells_w; RMNET_E_UNSUPPORTED for B or K > 65535;
 * RMNET_E_WORKSPACE for a NULL workspace or one shorter than rmnet_region_map_workspace_bytes(B, K, H, W), which needs
 * no initialisation.  Nothing is written on any refusal.
 * ------------------------------------------------------------------------------------------- */
size_t rmnet_region_map_workspace_bytes(int B, int K, int H, int W);
int rmnet_region_map_f32(const float *mask, int B, int K, int H, int W, float prob_threshold,
                         int n_pts_threshold, int n_bbox_loose_pixels, float *att_map,
                         int32_t *bboxes, int32_t *cell_rects, int pad_l, int pad_t,
                         int cell_stride, int cells_h, int cells_w, void *workspace,
                         size_t workspace_bytes, void *stream);

/* A1 + G1 fused: the boxes of the FLOW-WARPED previous mask,
 *   RMNet.get_att_map(prev_mask, flow) = att_map_generator(warp(prev_mask, flow))
 * (models/rmnet.py:252-287), without materialising the warped mask: flow [B,2,H,W] fp32 (x then y
 * displacement in pixels), everything else as rmnet_region_map_f32.  The warp follows the arithmetic
 * PyTorch-ROCm executes for warp(): bilinear, align_corners=True, zero padding, validity of the
 * sampling footprint thresholded at 0.9999.  `warped` (optional, [B,K,H,W], channel 0 untouched)
 * receives the warped mask itself.  Same workspace size and argument rules as rmnet_region_map_f32; a NULL flow is
 * RMNET_E_INVALID_ARG, with or without `warped`. */
int rmnet_region_map_warped_f32(const float *mask, const float *flow, int B, int K, int H, int W,
                                float prob_threshold, int n_pts_threshold, int n_bbox_loose_pixels,
                                float *att_map, int32_t *bboxes, int32_t *cell_rects, int pad_l,
                                int pad_t, int cell_stride, int cells_h, int cells_w, float *warped,
                                void *workspace, size_t workspace_bytes, void *stream);

/* Box -> cell rectangle only (same formula as above), for boxes already on the device. */
int rmnet_boxes_to_cell_rects_i32(const int32_t *bboxes, int n_boxes, int k_per_batch, int pad_l,
                                  int pad_t, int cell_stride, int cells_h, int cells_w,
                                  int32_t *cell_rects, void *stream);

/* ---------------------------------------------------------------------------------------------
 * M1 (+M2/M3 fused)  Regional memory read.
 * Replaces: MemoryReader.forward, models/rmnet.py:147-165 (bmm, /sqrt(De), softmax over THW,
 *           bmm, cat) and -- when rectangles are given -- the K/V box masking around it,
 *           models/rmnet.py:244-248 (memory side) and :356-358 (query side).
 *   m_key  [no, De, T, h, w]   element (o,c,t,y,x) at o*m_obj_stride + c*m_chan_stride + t*h*w + y*w + x
 *   m_val  [no, Do, T, h, w]   same strides rule with v_obj_stride / v_chan_stride
 *          (contiguous NCTHW: chan_stride = T*h*w, obj_stride = C*T*h*w; a pre-allocated memory
 *           bank of capacity Tcap uses chan_stride = Tcap*h*w).  Pass 0 to mean "contiguous".
 *   q_key  [no, De, h, w], q_val [no, Do, h, w]   contiguous
 *   mem_val [no, 2*Do, h, w]  out: channels [0,Do) = read-out, [Do,2Do) = q_val (masked if regional)
 *   p_out  [no, T*h*w, h*w] out or NULL: the softmax affinity the reference returns as `viz`
 *          (models/rmnet.py:157,165); computed only when requested (extra pass).
 *   mem_rects [no, T, 4] int32 or NULL; qry_rects [no, 4] int32 or NULL: cell rectangles
 *          (cx0,cx1,cy0,cy1) inclusive.  When given, cells outside a rectangle are treated as
 *          if K, V (memory) / q_key, q_val (query) had been multiplied by 0 there -- the inputs
 *          may be the un-masked tensors (the multiply is fused) or already masked ones.
 *          Both NULL = dense read (drop-in MemoryReader).
 *   flags  RMNET_MR_* below.
 * The fast path needs De == 128 and Do == 512 (RMNet's sizes, models/rmnet.py:185-186); other
 * sizes run a generic (slow, still on-GPU) path that needs the p-sized workspace.
 * Generic path: De <= 224 (RMNET_E_UNSUPPORTED beyond: its query tile lives in 64 KB of LDS), any Do; the same limit
 * holds for p_out at the fast shape, which that path computes.  Rectangles may stick out of the grid or be empty.
 * Fast path arithmetic: the memory is first staged (one launch, inside `workspace`) into a transient
 * split-fp16 bank (below) and read with 3-term fp16 MFMAs, fp32 accumulate -- fp32-class accuracy for
 * |K|, |V| < 1023.5.  The staging pass counts elements outside that window on the device; if there is
 * one (or a NaN / Inf), the exact-fp32 MFMA kernel (v_mfma_f32_16x16x4_f32, no range limit, ~4x slower)
 * does the read instead -- chosen on the device, no host synchronisation, no silent saturation.
 * RMNET_MR_EXACT_FP32 forces the exact kernel.  Parity with the reference is a tolerance (see tests).
 * RMNET_MR_F16 (opt-in) reads the staged bank with its hi planes only: K, V, the query and the soft-max weights enter
 * the MFMAs rounded to fp16 (11 significant bits), fp32 accumulate -- one MFMA term instead of three and half the bank
 * bytes, 1.5-2x as fast.  Error of a read-out: about 2^-11 of the values it averages (3e-4 relative at worst, a
 * peaked soft-max returning one cell's value; 5e-6 absolute when hundreds of cells contribute), against 1e-7 for the
 * default.  It meets the bar the reference's task sets (mask IoU within 1e-3 on whole clips, tests/test_gpu_parity.py);
 * it is NOT fp32-class.  Same range rules and the same device-side fallback as the default.
 * ------------------------------------------------------------------------------------------- */
#define RMNET_MR_DEFAULT 0
#define RMNET_MR_FORCE_GENERIC 1 /* use the generic path even for De=128, Do=512 (testing) */
#define RMNET_MR_EXACT_FP32 2    /* fast shape only: skip the split-fp16 bank, run the exact-fp32 MFMA kernel */
#define RMNET_MR_F16 4           /* fast shape only: fp16 operands (hi planes of the bank), fp32 accumulate */
#define RMNET_BANK_F16 4         /* the same switch for rmnet_bank_read_f32_at */
#define RMNET_MR_QX 8            /* fast shape only: RMNET_MR_F16 with an EXACT QUERY -- q enters the logits as a hi/lo pair (two MFMA terms), K, P
                                  * and V stay rounded to fp16.  q's rounding is the one logit error that is coherent over all memory cells of
                                  * a query; removing it recovers most of what RMNET_MR_F16 costs in mask IoU (measured on whole clips against
                                  * the CPU path: profiles/r05_iou_calibration.md) for 3 % (frame loop) to 9 % (back to back) of its speed.
                                  * Mutually exclusive with RMNET_MR_F16. */
#define RMNET_BANK_QX 8          /* the same switch for rmnet_bank_read_f32_at */

size_t rmnet_memory_read_workspace_bytes(int no, int De, int Do, int T, int h, int w, int flags);
int rmnet_memory_read_f32(const float *m_key, const float *m_val, const float *q_key,
                          const float *q_val, int no, int De, int Do, int T, int h, int w,
                          long long m_chan_stride, long long m_obj_stride, long long v_chan_stride,
                          long long v_obj_stride, float *mem_val, float *p_out,
                          const int32_t *mem_rects, const int32_t *qry_rects, int flags,
                          void *workspace, size_t workspace_bytes, void *stream);

/* Same call, with optional HIP events recorded on `stream` around the two kernels of the fast
 * path: ev_start at the very start of the call (before the staging pass), ev_mid after the read kernel, ev_end after the combine kernel of the exact-fp32
 * path (which returns at once when the split-fp16 bank kernel did the whole read)
 * (each a hipEvent_t as void*, any may be NULL).  bench.py uses this to time the dominant kernel
 * on the stream it actually runs on; it changes nothing else. */
int rmnet_memory_read_f32_ev(const float *m_key, const float *m_val, const float *q_key,
                             const float *q_val, int no, int De, int Do, int T, int h, int w,
                             long long m_chan_stride, long long m_obj_stride,
                             long long v_chan_stride, long long v_obj_stride, float *mem_val,
                             float *p_out, const int32_t *mem_rects, const int32_t *qry_rects,
                             int flags, void *workspace, size_t workspace_bytes, void *stream,
                             void *ev_start, void *ev_mid, void *ev_end);

/* Gradients of rmnet_memory_read_f32 (csrc/memory_read_bwd.hip): what loss.backward() sends through MemoryReader.forward
 * (models/rmnet.py:147-165 with the box masking of :244-248 / :356-358) in the reference's training loop.
 *   m_key, m_val, q_key, q_val, the sizes, strides and rectangles: the forward's arguments, unchanged.
 *   mem_val       [no, 2*Do, h, w]  the forward's output (its read-out half enters delta_n = sum_d G[d,n] R[d,n])
 *   grad_mem_val  [no, 2*Do, h, w]  the gradient that arrives
 *   d_m_key [no, De, T, h, w], d_m_val [no, Do, T, h, w]  out, addressed by m_key's / m_val's stride rule (a gradient buffer of
 *                 capacity Tcap is written in its first T frames only; frames >= T are not touched)
 *   d_q_key [no, De, h, w], d_q_val [no, Do, h, w]        out, contiguous
 * Any of the four gradient pointers may be NULL: that gradient is not computed, and the others have the same bits as in a
 * full call.  All four NULL is RMNET_E_INVALID_ARG.  Every element of a requested gradient is written: a cell outside its
 * rectangle gets 0.  The gradient is that of the EXACT function -- fp32 operands, fp32 accumulate on v_mfma_f32_16x16x4_f32,
 * P recomputed from per-query (max, sum) statistics -- whatever arithmetic produced mem_val.  No M x N matrix is written:
 * the workspace is linear in T*h*w + De*h*w + Do.  No atomics: two calls give the same bits.
 * One code path for De <= 224 (RMNET_E_UNSUPPORTED beyond), any Do, any T, h, w.  Other codes as rmnet_memory_read_f32:
 * RMNET_E_INVALID_ARG for a NULL input, a non-positive size, a channel stride below T*h*w, one rectangle array without the
 * other; RMNET_E_WORKSPACE for a NULL or short workspace.  With De > 96 the gradient kernels ask for more than 64 KB of
 * dynamic LDS: the first call on a device must not come from a stream that is capturing (RMNET_E_UNSUPPORTED). */
size_t rmnet_memory_read_backward_workspace_bytes(int no, int De, int Do, int T, int h, int w);
int rmnet_memory_read_backward_f32(const float *m_key, const float *m_val, const float *q_key, const float *q_val,
                                   int no, int De, int Do, int T, int h, int w,
                                   long long m_chan_stride, long long m_obj_stride, long long v_chan_stride,
                                   long long v_obj_stride, const float *mem_val, const float *grad_mem_val,
                                   const int32_t *mem_rects, const int32_t *qry_rects, float *d_m_key, float *d_m_val,
                                   float *d_q_key, float *d_q_val, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * P1/P2 + M1-M3  Regional memory BANK: the form the frame loop uses.
 * Replaces: the K-slot padding, box masking and per-frame torch.cat of the whole memory
 *           (models/rmnet.py:191-205, 239-248, 416-426) plus the read itself (:361).
 * A bank is an opaque device buffer of rmnet_bank_bytes(no, Tcap, h, w) bytes holding, per object
 * and per memorised frame ("slot"), only the cells inside that frame's box, already split into
 * fp16 hi/lo planes in the MFMA fragment order, plus the slot's per-channel value sums (see
 * csrc/bank.hip).  De = 128, Do = 512.  THE CALLER ZERO-FILLS A NEW BANK (it carries an overflow word and
 * the read kernel's arrival tickets, which every read leaves at zero again).
 *   rmnet_bank_append_f32: write frame `slot` from k4 [no,128,h,w] / v4 [no,512,h,w] (fp32, the
 *       KeyValue outputs, UN-masked) and its cell rectangles rects [no,4] (NULL = whole frame).
 *       A slot may be overwritten (the tentative "previous frame" slot of models/rmnet.py:416-426).
 *   rmnet_bank_read_f32: read the first T slots with q_key [no,128,h,w], q_val [no,512,h,w] and
 *       query rectangles qry_rects [no,4] (NULL = all cells) -> mem_val [no,1024,h,w], identical in
 *       meaning to rmnet_memory_read_f32 with the same rectangles.  Arithmetic: split-fp16 MFMA
 *       (hi*hi + hi*lo + lo*hi), fp32 accumulate -- fp32-class accuracy.  ONE kernel launch per 64 objects
 *       does the whole of MemoryReader.forward (soft-max read, merge of the partial results by the last
 *       workgroup of each query tile, the read-out of masked query cells, the q_val half of the cat).
 *       The bank is not const: the launch uses its ticket words -- one stream at a time may read a given bank.
 *       ev_* as in rmnet_memory_read_f32_ev (may be NULL; ev_mid and ev_end now bracket nothing).
 * Range: K and V are stored times 2^6; elements with |x| >= 1023.5 saturate and NaN / Inf are lost.  Every
 *       16-byte group written with such an element increments the int32 overflow word that lives at byte
 *       rmnet_bank_overflow_offset() of the bank; a caller that cannot rule such inputs out checks it (once per
 *       clip is enough) and re-runs with rmnet_memory_read_f32(..., RMNET_MR_EXACT_FP32).
 *       The QUERY is split the same way after scaling by log2(e)/sqrt(128) * 2^6 (about 8.2): a q_key element inside the query box
 *       with |x| beyond ~8e3 (or NaN / Inf) is counted in the same overflow word by the read itself (ABI v4; it used to saturate
 *       silently), so "overflow word == 0 after the read" covers both sides.  The word also carries two sticky error bits:
 *       1 << 30 = an append / read through a device counter hit a slot or frame count outside [0, Tcap] (nothing was written /
 *       the count was clamped), 1 << 29 = a merge inside a read gave up waiting for another workgroup's partial (cannot happen on
 *       a healthy device; the int32 right behind the overflow word counts these time-outs separately; the read-out of the pair whose
 *       merge gave up is written as NaN, never as a partially merged value).  Any non-zero value means: do not trust the reads of
 *       this bank, re-run exactly.  The word is a FLAG (zero / non-zero), not a count of elements: the read adds to it once per
 *       (query element, segment of the launch plan) that sees it, the append once per 16-byte group.
 *       Logit word (ABI v6): the THIRD int32 of the control block (byte rmnet_bank_overflow_offset() + 8) holds, as float bits, the
 *       largest soft-max reference max_j S_ij * log2(e) any read of this bank has used so far (sticky maximum over reads, queries and
 *       objects; >= 0; the kernel's reference is deferred: the true maximum logit lies within 8 above value * ln 2).  The error of
 *       RMNET_BANK_F16 / RMNET_BANK_QX grows with the logits (K and q are rounded to 11 bits: ~2^-11 |S| per logit), so a caller that
 *       wants the fp32-class result on peaked soft-maxes checks this word once per clip and re-reads with flags = 0 when it is large
 *       (rmnet_amd/rmnet.py does, bound and evidence: profiles/r06_iou_temperature.md).  Zero in a new bank.
 *       rmnet_bank_area_offset(): byte offset of the int32 [no][Tcap] table of cells stored per slot (accounting).
 *       One launch reads at most 2048 slots (LDS prefix arrays).  Longer memories (models/rmnet.py:416-426 has no bound; ABI v4):
 *       a bank may have any Tcap; rmnet_bank_read_f32 / _at with T > 2048 (host-side T only: T_dev must be NULL for such a bank)
 *       read it in chunks of 2048 slots and merge the chunks' read-outs by their soft-max state (m, l) -- the same merge the
 *       kernel applies to the partial results of one launch -- in a workspace of rmnet_bank_read_workspace_bytes_for(...) bytes.
 * rmnet_bank_read_f32_at(..., flags): 0 = the arithmetic above; RMNET_BANK_F16 = hi planes only (see RMNET_MR_F16: fp16
 *       operands, fp32 accumulate, ~2^-11 relative, 1.5-2x as fast); RMNET_BANK_QX = the same with an exact query (see
 *       RMNET_MR_QX).  The bank is the same in every mode: a clip can be memorised once and read in all three.
 * ------------------------------------------------------------------------------------------- */
size_t rmnet_bank_bytes(int no, int Tcap, int h, int w);
size_t rmnet_bank_overflow_offset(int no, int Tcap, int h, int w);
size_t rmnet_bank_area_offset(int no, int Tcap, int h, int w);
int rmnet_bank_append_f32(void *bank, int no, int Tcap, int h, int w, int slot, const float *k4,
                          const float *v4, const int32_t *rects, void *stream);
/* The same two calls with a DEVICE-RESIDENT frame counter (int32, may be NULL): the slot written is slot + *slot_dev,
 * the frames read are T + *T_dev (clamped to [1, Tcap]).  The host need not know how long the memory is, so one
 * captured HIP graph of the frame loop (models/rmnet.py:410-450: memorise frame t-1 into slot `committed`, read
 * committed + 1 frames) can be replayed for every frame while the counter is bumped by a one-element add between
 * replays. */
int rmnet_bank_append_f32_at(void *bank, int no, int Tcap, int h, int w, int slot, const int32_t *slot_dev,
                             const float *k4, const float *v4, const int32_t *rects, void *stream);
int rmnet_bank_read_f32_at(void *bank, int no, int Tcap, int h, int w, int T, const int32_t *T_dev, int flags,
                           const float *q_key, const float *q_val, const int32_t *qry_rects,
                           float *mem_val, void *workspace, size_t workspace_bytes, void *stream,
                           void *ev_start, void *ev_mid, void *ev_end);
/* workspace of a read: the first form covers T <= 2048 frames, the _for form any T (ABI v4, chunked reads) */
size_t rmnet_bank_read_workspace_bytes(int no, int h, int w);
size_t rmnet_bank_read_workspace_bytes_for(int no, int h, int w, int T);
int rmnet_bank_read_f32(void *bank, int no, int Tcap, int h, int w, int T,
                        const float *q_key, const float *q_val, const int32_t *qry_rects,
                        float *mem_val, void *workspace, size_t workspace_bytes, void *stream,
                        void *ev_start, void *ev_mid, void *ev_end);

/* M2/M3 standalone: y = x * rectangle-mask, x [n, C, T, h, w] contiguous, rects [n, T, 4].
 * Replaces the elementwise multiplies at models/rmnet.py:247-248 and :357-358 when a caller
 * wants the masked tensors themselves (e.g. RMNet.memorize's return values). */
int rmnet_rect_mask_f32(const float *x, int n, int C, int T, int h, int w, const int32_t *rects,
                        float *y, void *stream);

/* C1 glue: per-channel affine + residual + ReLU in one pass over an NCHW fp32 activation,
 *   out[n,c,:] = act(x[n,c,:] * scale[c] + shift[c] + (res[n,c,:] * res_scale[c] + res_shift[c]))
 * scale / shift / res / res_scale / res_shift may each be NULL (1, 0, no residual, 1, 0); act = relu:
 * 0 none, 1 ReLU (NaN propagates like torch.relu), 2 LeakyReLU(0.1) (the slope of every activation of
 * models/tiny_flownet.py).  In place (out == x or out == res) is allowed.
 * Replaces the elementwise passes the reference runs after every convolution in eval mode:
 * BatchNorm2d + ReLU + skip add of the torchvision Bottleneck (models/rmnet.py:66-80, 96-103 use
 * resnet50's layers) and conv bias + ReLU + skip add of ResBlock (models/rmnet.py:24-48), with
 * scale/shift = gamma/sqrt(var+eps), beta - mean*scale  or  (NULL, conv bias). */
int rmnet_channel_affine_f32(const float *x, const float *scale, const float *shift,
                             const float *res, const float *res_scale, const float *res_shift,
                             int relu, long long N, int C, long long HW, float *out, void *stream);

/* C1 glue: out = max_pool2d(relu(x * scale[c] + shift[c]), kernel 3, stride 2, padding 1), x [N,C,H,W] ->
 * out [N,C,(H-1)/2+1,(W-1)/2+1] fp32 NCHW; scale / shift may be NULL.  Replaces bn1 -> relu -> maxpool of
 * the ResNet-50 stems (torchvision layers used at models/rmnet.py:74-76, 98-100) without writing the
 * full-resolution activation. */
int rmnet_affine_relu_maxpool_f32(const float *x, const float *scale, const float *shift, long long N,
                                  int C, int H, int W, float *out, void *stream);

/* C1 glue: out = skip + bilinear_x2(x), x [N,C,h,w] -> out / skip [N,C,2h,2w] fp32 NCHW, with
 * torch's align_corners=False source-index rule.  skip may be NULL (plain upsample); out may be skip.
 * Replaces F.interpolate(pm, scale_factor=2, mode='bilinear') and the add of Refine.forward
 * (models/rmnet.py:117-119). */
int rmnet_upsample2x_add_f32(const float *x, const float *skip, long long N, int C, int h, int w,
                             float *out, void *stream);

/* C1 glue, CHANNELS-LAST variants (ABI v6): the same three passes for activations that are [N, H, W, C] in memory -- what MIOpen's NHWC
 * convolution kernels produce and consume without layout transposes (torch: tensor.to(memory_format=torch.channels_last)).  Same arithmetic and
 * rounding as the NCHW entries above; C % 4 == 0, every pointer 16-byte aligned (RMNET_E_INVALID_ARG otherwise).
 *   rmnet_channel_affine_nhwc_f32:      x / res / out [rows = N*H*W][C]
 *   rmnet_upsample2x_add_nhwc_f32:      x [N,h,w,C] -> out / skip [N,2h,2w,C]
 *   rmnet_affine_relu_maxpool_nhwc_f32: x [N,H,W,C] -> out [N,(H-1)/2+1,(W-1)/2+1,C] */
int rmnet_channel_affine_nhwc_f32(const float *x, const float *scale, const float *shift, const float *res, const float *res_scale,
                                  const float *res_shift, int relu, long long rows, int C, float *out, void *stream);
int rmnet_upsample2x_add_nhwc_f32(const float *x, const float *skip, long long N, int C, int h, int w, float *out, void *stream);
int rmnet_affine_relu_maxpool_nhwc_f32(const float *x, const float *scale, const float *shift, long long N, int C, int H, int W,
                                       float *out, void *stream);

/* C1 decoder convolutions (additive export, same ABI version): 3x3 / stride 1 / pad 1 convolution with Cout = 256 on the fp16
 * MFMA pipes with split operands (csrc/conv3x3.hip): each fp32 operand is carried as fp16 hi + lo and each product keeps
 * Ah*Wh + Ah*Wl + Al*Wh with fp32 accumulation -- fp32-class arithmetic.  Replaces the 256-channel convolutions of the decoder
 * (models/rmnet.py:107-140: Decoder.convFM, Decoder.ResMM, Refine.convFS / ResFS / ResMM) together with their bias / ReLU / skip.
 *   x    [N, H, W, Cin] fp32 (channels-last), Cin % 32 == 0;
 *   out  [N, H, W, 256] fp32 = act(conv(pre(x)) + bias[co] + res), pre = ReLU when RMNET_CONV_RELU_IN, act = ReLU when
 *        RMNET_CONV_RELU_OUT; bias [256] and res [N, H, W, 256] may be NULL.  out must not overlap x; it may be res itself.
 *   wpack, w_unscale: the packed weights (layout below);
 *   range_word: device int32, may be NULL.  Activations are split after a scaling by 2^6 (exact), so |pre(x)| must be below
 *        65504 / 64 = 1023.5; every element outside (or NaN / Inf) is saturated and ADDED to *range_word (once per element).
 *        A non-zero word means the output is not fp32-class: the caller checks it (no host synchronisation here).
 * Every pointer 16-byte aligned.  RMNET_E_UNSUPPORTED for Cin % 32 != 0 or N*H*W*max(Cin, 256) >= 2^31.
 *
 * Weight pack (built by the caller; rmnet_amd.ops.conv3x3_pack does it in torch) for w [256][Cin][3][3] fp32:
 *   e[co]          = 15 - ceil-exponent of max |w[co]|, i.e. max |w[co]| * 2^e[co] lies in [2^14, 2^15) (e = 0 for a zero channel);
 *   ws             = w[co][ci][ky][kx] * 2^e[co] (exact),  hi = fp16_rne(ws),  lo = fp16_rne(ws - hi);
 *   wpack          fp16 [9][Cin / 32][2][256][32]: [tap = 3 * ky + kx][ci / 32][plane: hi, lo][co][ci % 32]  (18 * Cin * 256 * 2 bytes);
 *   w_unscale[co]  fp32 = 2^-e[co]. */
#define RMNET_CONV_RELU_IN 1
#define RMNET_CONV_RELU_OUT 2
int rmnet_conv3x3_split_f32(const float *x, const void *wpack, const float *w_unscale, const float *bias, const float *res, int flags,
                            int N, int H, int W, int Cin, float *out, int32_t *range_word, void *stream);

/* The same convolution on the kernel that stages the weights through LDS (additive export, same ABI version): the arguments,
 * argument rules and return codes of rmnet_conv3x3_split_f32, and its results bit for bit, range word included.
 * rmnet_conv3x3_split_f32 runs conv3x3_wreg, whose waves load their weight fragments straight from the pack into registers;
 * this entry runs conv3x3_split, the kernel that entry ran before, and is kept for A/B measurements and as the reference of
 * tests/test_conv3x3_wreg.py (rmnet_amd.ops.conv3x3_split selects it with RMNET_CONV3X3_KERNEL=lds). */
int rmnet_conv3x3_split_lds_f32(const float *x, const void *wpack, const float *w_unscale, const float *bias, const float *res,
                                int flags, int N, int H, int W, int Cin, float *out, int32_t *range_word, void *stream);

/* The same convolution for Cin = 256 on the kernel that stages a whole tap row of activations in LDS once (additive export, same
 * ABI version; csrc/conv3x3_rows.hip: conv3x3_rows): the arguments, argument rules and return codes of rmnet_conv3x3_split_f32, and
 * its results bit for bit, range word included -- the K order per accumulator, the operand bits and the epilogue are the same.
 * Additionally RMNET_E_UNSUPPORTED unless Cin == 256 (the row image, 130 pixels x 256 channels x hi / lo, is what fits a CU's
 * LDS), and nothing is written then.  The kernel asks for 137216 B of dynamic LDS, which needs a function attribute: it is set at
 * the first call on a device, and that first call must not come from a stream that is capturing (RMNET_E_UNSUPPORTED): call once
 * eagerly before capturing.  rmnet_amd.ops.conv3x3_split selects this entry with RMNET_CONV3X3_ROWS when RMNET_CONV3X3_KERNEL is
 * not set. */
int rmnet_conv3x3_rows_f32(const float *x, const void *wpack, const float *w_unscale, const float *bias, const float *res, int flags,
                           int N, int H, int W, int Cin, float *out, int32_t *range_word, void *stream);

/* C1b gradients of the decoder convolutions (additive exports, same ABI version; csrc/conv3x3_wgrad.hip).
 *
 * The data gradient needs no entry of its own: for stride 1 / pad 1 it is rmnet_conv3x3_split_f32 on the gradient with the pack of
 * the transposed, flipped weight (rmnet_amd.ops.conv3x3_dgrad_pack).  The weight and bias gradient is
 *   dw[co][ky][kx][ci] = (sum over n, y, x of  g[n, y, x, co] * pre(x)[n, y + ky - 1, x + kx - 1, ci]) / (g_scale[0] * g_scale[1])
 *   db[co]             = (sum over n, y, x of  g[n, y, x, co]) / (g_scale[0] * g_scale[1])
 * with zeros outside the map and pre = ReLU under RMNET_CONV_RELU_IN (the only flag), in the three-term split-fp16 arithmetic of
 * the forward with the pixel as reduction index.
 *   x        [N, H, W, Cin] fp32 (channels-last), Cin % 32 == 0: the forward's input, split as the forward splits it (x 2^6, the
 *            window |pre(x)| < 1023.5);
 *   g        [N, H, W, 256] fp32: the gradient of the convolution's output AFTER staging, i.e. times the power of two
 *            g_scale[0] * g_scale[1] that puts its largest element into [2^8, 2^9) (rmnet_conv_grad_stage_f32); it is split like x,
 *            so |g| must be below 1023.5 as well;
 *   g_scale  device pointer to two fp32 powers of two whose product is the staging scale; both are undone exactly when dw and db
 *            are written ({1, 1} for a gradient that was not staged).  Nothing is read on the host;
 *   dw       fp32, 9 * Cin * 256 elements in the channels-last strides of a [256, Cin, 3, 3] tensor: [co][ky][kx][ci];
 *   db       fp32 [256], may be NULL;
 *   workspace  rmnet_conv3x3_wgrad_workspace_bytes(N, H, W, Cin) bytes (0 for a shape the entry refuses): the pixel axis is cut into
 *            ranges, each range's partial dw / db goes here and a merge kernel adds them in range order.  No atomics: every element
 *            of dw and db is written exactly once and two calls return the same bits;
 *   range_word  device int32, may be NULL: elements of pre(x) and of g outside the window (NaN / Inf included) are saturated and
 *            added to it, once per element and call (the data gradient's calls of rmnet_conv3x3_split_f32 count g again, once
 *            per call: a bad element of g is counted 1 + Cin / 256 times by a full backward).
 * Every pointer 16-byte aligned (range_word: 4).  dw, db and the workspace must not overlap x, g, g_scale, range_word or each other.
 * RMNET_E_INVALID_ARG for a NULL x, g, g_scale or dw, a non-positive size, another flag, a misaligned pointer or an overlap;
 * RMNET_E_UNSUPPORTED for Cin % 32 != 0, W > 448 (the activation image of a pixel range and its halo of W + 1 pixels on either side
 * must fit a CU's LDS) or N*H*W*max(Cin, 256) >= 2^31; RMNET_E_WORKSPACE for a NULL or short workspace -- all before anything is
 * launched.  The kernel asks for more than 64 KB of dynamic LDS, which needs a function attribute: it is set at the first call on
 * a device, and that first call must not come from a stream that is capturing (RMNET_E_UNSUPPORTED): call once eagerly before
 * capturing. */
size_t rmnet_conv3x3_wgrad_workspace_bytes(int N, int H, int W, int Cin);
int rmnet_conv3x3_wgrad_f32(const float *x, const float *g, const float *g_scale, int flags, int N, int H, int W, int Cin, float *dw,
                            float *db, void *workspace, size_t workspace_bytes, int32_t *range_word, void *stream);

/* The stage pass in front of the two gradient GEMMs: one elementwise kernel, no host synchronisation.
 *   gs[i] = (act == NULL || act[i] > 0 ? g[i] : 0) * 2^s        s = 9 - e for *amax in [2^(e-1), 2^e), so that 2^s *amax lies in
 *   [2^8, 2^9); s = 0 when *amax is 0, NaN or Inf.  g_scale[0] * g_scale[1] = 2^s: g_scale[0] = 2^min(s, 126), g_scale[1] the rest
 *   (1 unless *amax < 2^-118, where 2^s is no fp32 number).
 * g, gs (and act) hold n floats, n % 4 == 0, 16-byte aligned; gs may be g itself.  *amax (device, 4-byte aligned) is an upper bound
 * of |g[i]| taken before the mask; g_scale (device, 16-byte aligned) receives the two floats.  act is the forward's output under
 * RMNET_CONV_RELU_OUT, else NULL.  RMNET_E_INVALID_ARG for a NULL g / amax / gs / g_scale, n < 1, n % 4 != 0, a misaligned pointer
 * or an overlap other than gs == g; RMNET_E_UNSUPPORTED for n >= 2^31. */
int rmnet_conv_grad_stage_f32(const float *g, const float *act, const float *amax, long long n, float *gs, float *g_scale,
                              void *stream);

/* C1c gradients of the key / value heads (additive exports, same ABI version; csrc/conv_wgrad_n.hip).
 *
 * rmnet_conv3x3_wgrad_n_f32 is rmnet_conv3x3_wgrad_f32 for a gradient g [N, H, W, Cout] with Cout % 128 == 0: dw holds
 * 9 * Cin * Cout elements as [co][ky][kx][ci], db [Cout] or NULL.  The same arithmetic element for element; the output channels are
 * walked in tiles of 256 (the last one may hold 128) and the pixel ranges are planned for Cin / 16 * ceil(Cout / 256) workgroups
 * each, so Cout == 256 returns the bits of rmnet_conv3x3_wgrad_f32 in dw, db and the range word.  Every rule of that entry holds
 * with Cout in place of 256 (alignment, overlaps, RMNET_E_WORKSPACE against rmnet_conv3x3_wgrad_n_workspace_bytes, W <= 448,
 * N*H*W*max(Cin, Cout) < 2^31 and 9*Cin*Cout < 2^31, the first call on a device outside capture); Cout <= 0 is
 * RMNET_E_INVALID_ARG, Cout % 128 != 0 RMNET_E_UNSUPPORTED.  An element of g or pre(x) outside the window is counted once. */
size_t rmnet_conv3x3_wgrad_n_workspace_bytes(int N, int H, int W, int Cin, int Cout);
int rmnet_conv3x3_wgrad_n_f32(const float *x, const float *g, const float *g_scale, int flags, int N, int H, int W, int Cin, int Cout,
                              float *dw, float *db, void *workspace, size_t workspace_bytes, int32_t *range_word, void *stream);

/* The stage pass for a gradient that the memory read hands back: one launch, no host synchronisation.
 *   gs[n, y, x, c] = g[n, c, y, x] * 2^s   where (x, y) lies inside image n's rectangle rects[n] = (cx0, cx1, cy0, cy1), inclusive
 *                                          (clamped to the map, the convention of rmnet_conv_split_region_f32);
 *                  = +0.0                  elsewhere: a select, whatever g holds there (NaN and Inf included) does not reach gs.
 * rects NULL: every cell is inside.  s, *amax (taken before the mask) and g_scale are those of rmnet_conv_grad_stage_f32.
 * gs is dense channels-last [N, H, W, C], C % 4 == 0.  layout says how g is laid out:
 *   RMNET_GRAD_LAYOUT_NHWC    dense channels-last like gs (sn and sc are not looked at); gs may be g itself;
 *   RMNET_GRAD_LAYOUT_PLANES  element (n, c, y, x) at g[n * sn + c * sc + y * W + x], sc >= H*W, sn >= (C - 1) * sc + H*W: an NCHW
 *                             tensor, one tensor of the regional pair, a [:, :, t] slice of [N, C, T, H, W].
 * gs and g_scale 16-byte aligned, g 16 (NHWC) or 4 (planes), amax and rects 4.  RMNET_E_INVALID_ARG for a NULL g / amax / gs /
 * g_scale, a non-positive size, another layout, a misaligned pointer, planes that fold onto each other, or gs / g_scale
 * overlapping an input (other than gs == g, NHWC) or each other; RMNET_E_UNSUPPORTED for C % 4 != 0 or 2^31 floats or more in gs
 * or spanned by g. */
#define RMNET_GRAD_LAYOUT_NHWC 0
#define RMNET_GRAD_LAYOUT_PLANES 1
int rmnet_conv_grad_stage_rect_f32(const float *g, int layout, long long sn, long long sc, const int32_t *rects, const float *amax,
                                   int N, int C, int H, int W, float *gs, float *g_scale, void *stream);

/* C1 trunk / key-value convolutions (additive export, same ABI version): the arithmetic, range word and flags of
 * rmnet_conv3x3_split_f32 for kernel size ksize = 1 or 3 (padding ksize / 2), stride 1 or 2 and Cout % 64 == 0 (csrc/conv_split.hip).
 * Replaces the ResNet-50 bottleneck convolutions (BatchNorm folded into the pack, skip add and ReLU in the epilogue) and the two
 * KeyValue heads (one launch over their concatenated weights).
 *   x     [N, H, W, Cin] fp32 (channels-last), Cin % 32 == 0;
 *   out   [N, Ho, Wo, Cout] fp32 = act(conv(pre(x)) + shift[co] + res), Ho = (H + 2 * pad - ksize) / stride + 1 (Wo alike);
 *         shift [Cout] and res [N, Ho, Wo, Cout] may be NULL; out must not overlap x, it may be res itself;
 *   out2  NULL, or two outputs: channels [0, out_split) go to out [N, Ho, Wo, out_split] and [out_split, Cout) to
 *         out2 [N, Ho, Wo, Cout - out_split] (0 < out_split < Cout, out_split % 4 == 0, res NULL, no overlap with x or out);
 *   range_word: as above, each input element the convolution reads counted once (by the workgroups of the first Cout tile).
 * Every pointer 16-byte aligned.  RMNET_E_UNSUPPORTED for another ksize / stride, Cin % 32 != 0, Cout % 64 != 0, or
 * N*H*W*Cin or N*Ho*Wo*Cout >= 2^31.
 *
 * Weight pack (rmnet_amd.ops.conv_split_pack) for w [Cout][Cin][ksize][ksize] fp32 and an optional per-channel factor g [Cout]
 * (the folded BatchNorm scale; 1 when absent):
 *   wg             = w[co] * g[co] formed in float64;
 *   e[co]          = 15 - ceil-exponent of max |wg[co]| (e = 0 for a zero channel);
 *   ws             = wg * 2^e[co] (exact),  hi = fp16_rne(ws),  lo = fp16_rne(ws - hi)  (hi + lo = wg * 2^e to ~2^-22 relative);
 *   wpack          fp16 [ksize^2][Cin / 32][2][Cout][32]: [tap = ksize * ky + kx][ci / 32][plane: hi, lo][co][ci % 32];
 *   w_unscale[co]  fp32 = 2^-e[co].  For ksize 3 and Cout 256 without g this is rmnet_conv3x3_split_f32's pack. */
int rmnet_conv_split_f32(const float *x, const void *wpack, const float *w_unscale, const float *shift, const float *res, int flags,
                         int N, int H, int W, int Cin, int Cout, int ksize, int stride, float *out, float *out2, int out_split,
                         int32_t *range_word, void *stream);

/* C1 pre-split activations (additive export, same ABI version).  rmnet_conv_split_f32 splits every activation it reads at every tap
 * and in every Cout tile; the split depends on the element alone, so a tensor that only such convolutions read can be kept in split
 * form and split once (csrc/conv_split.hip: the XS / OS instances of the one kernel template conv_split, and split_act).
 *
 * The split ACTIVATION form of an NHWC activation v [M][C] fp32, C % 32 == 0, is [M][C / 32][2][32] fp16: per pixel and block of 32
 * channels the 32 hi halves, then the 32 lo halves, of
 *     y = pre(v) * 64;  c = fminf(fmaxf(y, -65504), 65504);  hi = (fp16)c;  lo = (fp16)(c - (float)hi)
 * (pre = an optional ReLU that keeps NaN; float32 arithmetic, round to nearest even; hi + lo == c to 2^-22 relative).  It has 4 bytes
 * per element like fp32, a pixel has the same byte stride, and every aligned 16-byte chunk holds 8 halves of one plane.  An element
 * with !(fabsf(y) <= 65504) adds one to the range word where the form is PRODUCED, once; a consumer counts nothing.
 *
 * rmnet_conv_split_pre_f32: rmnet_conv_split_f32 with two more flag bits -- the same kernel template, so the same tiles, arithmetic,
 * K order, epilogue and results; both entries share one set of argument rules.
 *   RMNET_CONV_X_SPLIT    x is in split form.  RMNET_CONV_RELU_IN is then refused (the producer applied it), and the convolution
 *                         adds nothing to the range word for its input;
 *   RMNET_CONV_OUT_SPLIT  out receives act(conv + shift + res) in split form instead of fp32 and the elements of it outside the
 *                         window are counted.  out2 must be NULL, and out must overlap neither x nor res (an fp32 out may still BE
 *                         res).
 *   With neither bit the call is rmnet_conv_split_f32's.  Other argument rules and return codes: as there.
 * rmnet_split_act_f32: x [M][C] fp32 -> out in split form, ReLU first when relu != 0, for tensors that another kernel produced.
 *   One grid-stride launch, no LDS.  x and out 16-byte aligned and not overlapping (RMNET_E_INVALID_ARG); RMNET_E_UNSUPPORTED for
 *   C % 32 != 0. */
#define RMNET_CONV_X_SPLIT 4
#define RMNET_CONV_OUT_SPLIT 8
int rmnet_conv_split_pre_f32(const void *x, const void *wpack, const float *w_unscale, const float *shift, const float *res, int flags,
                             int N, int H, int W, int Cin, int Cout, int ksize, int stride, void *out, float *out2, int out_split,
                             int32_t *range_word, void *stream);
int rmnet_split_act_f32(const float *x, long long M, int C, int relu, void *out, int32_t *range_word, void *stream);

/* The key / value heads of the frame step on the cells that the regional memory uses (additive export, same ABI version;
 * csrc/conv_split.hip: conv_split_region, the RG instance of the kernel's body).  The convolution of rmnet_conv_split_pre_f32 with
 * RMNET_CONV_X_SPLIT and two outputs, computed only for the cells inside one rectangle per image:
 *   rects [N][4] int32 (cx0, cx1, cy0, cy1), inclusive, on the device; clamped to the map exactly as the bank kernels clamp theirs
 *         (max(., 0), min(., W - 1 / H - 1)); cx1 < cx0 or cy1 < cy0 after that: an empty rectangle;
 *   out   [N, out_split, H, W] and out2 [N, Cout - out_split, H, W] fp32, NCHW (the layout rmnet_bank_append_f32_at and
 *         rmnet_bank_read_f32_at take).  A cell inside its image's rectangle holds the bits that rmnet_conv_split_pre_f32 gives it;
 *         every other cell is +0.0, written by this kernel: the outputs need no initialisation.
 * The GEMM's rows are the cells of all rectangles, image after image, each rectangle row-major; the tile is the 128 x 128 one, the K
 * order and the epilogue's arithmetic are those of the dense kernel.  The grid is the worst case, ceil(N*H*W / 128) x Cout / 128:
 * nothing is read back, and a workgroup past the last row only writes its share of the zeros.  x is in split form, so nothing is
 * added to the range word.
 * Rules: those of rmnet_conv_split_pre_f32, and RMNET_E_INVALID_ARG for rects == NULL or not 16-byte aligned, a flag other than
 * RMNET_CONV_X_SPLIT (required) and RMNET_CONV_RELU_OUT, out2 == NULL, or an output that overlaps rects; RMNET_E_UNSUPPORTED for
 * ksize != 3, stride != 1, Cout % 128 != 0 or N > 64 (the caller then runs the dense head). */
int rmnet_conv_split_region_f32(const void *x, const void *wpack, const float *w_unscale, const float *shift, int flags, int N, int H,
                                int W, int Cin, int Cout, int ksize, int stride, const int32_t *rects, float *out, float *out2,
                                int out_split, int32_t *range_word, void *stream);

/* The trunks' stride-1 3x3 bottleneck convolutions on the kernel that stages a whole tap row of activations in LDS once (additive
 * export, same ABI version; csrc/conv_rows.hip: conv_rows<C>): the arguments and argument rules of rmnet_conv_split_pre_f32, and its
 * results bit for bit, range word included -- the K order per accumulator, the operand bits and the epilogue are the same -- for
 *   ksize = 3, stride = 1, Cin == Cout in {64, 128, 256}, RMNET_CONV_X_SPLIT set (x in split form), out fp32 or, with
 *   RMNET_CONV_OUT_SPLIT, in split form, shift optional, RMNET_CONV_RELU_OUT optional, res == NULL and out2 == NULL.
 * Every other call that rmnet_conv_split_pre_f32 would accept returns RMNET_E_UNSUPPORTED and writes nothing.  A workgroup owns
 * 32768 / C consecutive pixels and all C channels; the kernel asks for up to 137216 B of dynamic LDS, which needs a function
 * attribute: it is set at the first call of an instance (C, output form) on a device, and that first call must not come from a
 * stream that is capturing (RMNET_E_UNSUPPORTED): call once eagerly before capturing.  rmnet_amd.ops.conv_split selects this entry
 * with RMNET_TRUNK_ROWS for the classes of ops.TRUNK_ROWS_CLASSES. */
int rmnet_conv_rows_pre_f32(const void *x, const void *wpack, const float *w_unscale, const float *shift, const float *res, int flags,
                            int N, int H, int W, int Cin, int Cout, int ksize, int stride, void *out, float *out2, int out_split,
                            int32_t *range_word, void *stream);

/* C1 encoder stems (additive export, same ABI version): the 7x7 / stride 2 / pad 3 stem convolution, the folded BatchNorm, ReLU and
 * MaxPool2d(3, stride 2, padding 1) in ONE launch (csrc/stem.hip), on the split-fp16 arithmetic of rmnet_conv3x3_split_f32; the
 * half-resolution 64-channel activation is never written.  Replaces conv1 (+ conv1_m + conv1_o) / bn1 / relu / maxpool of both
 * encoders (models/rmnet.py:66-76, 96-100) and the 5-channel concatenation in front of the memory encoder's stem.
 *   frame [N, 3, H, W] fp32 NCHW; mask, other [N, H, W] fp32, both may be NULL.  mask NULL: Cin = 3 (query encoder; other must be
 *         NULL too).  mask given: Cin = 5, input channels (frame 0..2, mask, other); other NULL = an all-zero fifth plane;
 *   out   [N, Hp, Wp, 64] fp32 (channels-last) = max_pool(relu(conv(x) * g + shift[co])), Hc = (H - 1) / 2 + 1, Hp = (Hc - 1) / 2 + 1
 *         (Wc, Wp alike); any H, W >= 1.  Pool padding counts as -inf; a NaN in a window gives NaN (as rmnet_affine_relu_maxpool_f32);
 *   shift [64] may be NULL; g is folded into the pack;
 *   range_word: as above; every INPUT element (of the planes given) with |x| >= 1023.5, NaN or Inf is saturated and counted once.
 * wpack, w_unscale, shift and out 16-byte aligned.  RMNET_E_UNSUPPORTED only for N*3*H*W or N*Hp*Wp*64 >= 2^31.
 *
 * Weight pack (rmnet_amd.ops.stem_pack) for w [64][Cin][7][7] fp32, Cin = 3 or 5 (the memory encoder: conv1 | conv1_m | conv1_o
 * stacked along Cin), and an optional per-channel factor g [64]:
 *   wg, e[co], ws, hi, lo, w_unscale: as for rmnet_conv_split_f32;
 *   k              = (7 * ky + kx) * Cin + ci, 0 <= k < 49 * Cin, zero-padded to Kp = 160 (Cin 3: 147) or 256 (Cin 5: 245);
 *   wpack          fp16 [Kp / 32][2][64][32]: [k / 32][plane: hi, lo][co][k % 32]  (Kp * 64 * 2 * 2 bytes). */
int rmnet_stem_split_f32(const float *frame, const float *mask, const float *other, const void *wpack, const float *w_unscale,
                         const float *shift, int N, int H, int W, float *out, int32_t *range_word, void *stream);

/* C2 TinyFlowNet's front end (additive export, same ABI version): zero-padding of the two frames, the bilinear halving, the 6-channel
 * concatenation, conv1 (7x7 / stride 2 / pad 3, 6 -> 64), its bias and LeakyReLU(0.1) in ONE launch (csrc/flow_stem.hip), on the
 * split-fp16 arithmetic of rmnet_stem_split_f32; neither the padded frames nor the half-resolution pair is written.  Replaces
 * pad_divide_by / F.interpolate / torch.cat / conv1 of TinyFlowNet._forward (models/tiny_flownet.py).
 *   img0, img1 [N, 3, H, W] fp32, read in place, 4-byte aligned: frame n is a dense [3, H, W] block at img + n * batch_stride
 *         floats (batch_stride0 / batch_stride1 >= 3*H*W, RMNET_E_INVALID_ARG otherwise), so frame t of a [N, T, 3, H, W] clip is
 *         read without a copy;
 *   Hpad, Wpad, lh, lw: the padded frame is [Hpad, Wpad] with the frame at rows lh .. lh+H-1 and columns lw .. lw+W-1 and zeros
 *         elsewhere (lh, lw >= 0, lh + H <= Hpad, lw + W <= Wpad; RMNET_E_INVALID_ARG otherwise).  Hh = Hpad / 2, Wh = Wpad / 2;
 *   pair  [N, 6, Hh, Wh] (never materialised): channel c < 3 from img0, 3 <= c < 6 from img1; element (Y, X) = 0.25 * ((p[2Y][2X] +
 *         p[2Y][2X+1]) + (p[2Y+1][2X] + p[2Y+1][2X+1])) of the padded frame p -- F.interpolate(scale_factor=0.5, 'bilinear');
 *   out   [N, Hc, Wc, 64] fp32 (channels-last) = leaky_0.1(conv7x7_s2_p3(pair) + bias[co]), Hc = (Hh - 1) / 2 + 1 (Wc alike);
 *         must not overlap img0 or img1 (RMNET_E_INVALID_ARG);
 *   bias  [64] may be NULL;
 *   range_word: as above; every element of PAIR with |x| >= 1023.5, NaN or Inf is saturated and counted once.
 * wpack, w_unscale, bias and out 16-byte aligned.  RMNET_E_UNSUPPORTED for an odd Hpad or Wpad and for N*3*H*W or N*Hc*Wc*64 >= 2^31;
 * nothing is written on any refusal.  The kernel asks for 115296 B of dynamic LDS, which needs a function attribute: it is set at the
 * first call on a device, and that first call must not come from a stream that is capturing (RMNET_E_UNSUPPORTED): call once eagerly
 * before capturing.
 *
 * Weight pack (rmnet_amd.ops.flow_stem_pack) for w [64][6][7][7] fp32: rmnet_stem_split_f32's layout with Cin = 6:
 *   k = (7 * ky + kx) * 6 + ci, 0 <= k < 294, zero-padded to Kp = 320;  wpack fp16 [10][2][64][32]  (81920 bytes). */
int rmnet_flow_stem_f32(const float *img0, const float *img1, long long batch_stride0, long long batch_stride1, const void *wpack,
                        const float *w_unscale, const float *bias, int N, int H, int W, int Hpad, int Wpad, int lh, int lw, float *out, int32_t *range_word, void *stream);

/* C1 decoder prediction head (additive export, same ABI version): out = conv3x3_p1(relu(x), w) + bias with two output channels in
 * plain fp32 FMA (csrc/pred_head.hip).  Replaces F.relu(m2), Decoder.pred2 (models/rmnet.py:138-139) and the layout copy behind it.
 *   x    [n, Hq, Wq, C] fp32 (channels-last), C % 32 == 0, 16-byte aligned;  w [2][C][3][3], bias [2] fp32 (no pack);
 *   out  [n, 2, Hq, Wq] fp32 NCHW.
 * No window and no range word.  RMNET_E_UNSUPPORTED for C % 32 != 0 or n*Hq*Wq*C >= 2^31. */
int rmnet_pred_head_f32(const float *x, const float *w, const float *bias, int n, int Hq, int Wq, int C, float *out, void *stream);

/* C2 TinyFlowNet's wide convolutions (additive export, same ABI version): the arithmetic and range word of rmnet_conv_split_f32 over a
 * tap list (csrc/flow_conv.hip), for forward convolutions with ksize = 3 or 5 (padding ksize / 2), stride 1 or 2, and -- with
 * RMNET_FLOW_TRANSPOSED -- for ConvTranspose2d(4, stride 2, padding 1) (ksize 4, stride 2) as four 2x2-tap phases, one per output
 * parity.  Input and output carry a channel stride, so that a layer reads and writes concatenation buffers in place.  Replaces
 * conv2 .. conv5_1 and deconv4 .. deconv2 of TinyFlowNet (models/tiny_flownet.py) with their bias + LeakyReLU(0.1) and the torch.cat
 * of their outputs.
 *   x     [N, H, W, x_ld] fp32: channels 0 .. Cin-1 of every pixel are the input; x_ld % 4 == 0, x_ld >= ceil32(Cin) (Cin rounded up
 *         to a multiple of 32).  Channels Cin .. ceil32(Cin)-1 are read and multiplied by the pack's zero weights: any bit pattern;
 *   out   [N, Ho, Wo, out_ld] fp32: channels coff .. coff+Cout-1 of every pixel = act(conv(x) + shift[co]); no other byte is
 *         written.  out_ld % 4 == 0, coff % 4 == 0, coff + Cout <= out_ld.  Ho = (H + 2 * pad - ksize) / stride + 1, or 2 * H
 *         transposed (Wo alike).  act: none, ReLU (RMNET_FLOW_RELU) or y > 0 ? y : y * 0.1f (RMNET_FLOW_LEAKY); not both.
 *         shift [Cout] may be NULL.  The byte ranges of x and out (whole strided buffers) must not overlap;
 *   range_word: device int32, may be NULL.  Elements of the channels 0 .. Cin-1 with |x| >= 1023.5, NaN or Inf are saturated and
 *         counted, once per tap that reads them (so possibly several times): zero means no such element was read.
 * x, wpack, w_unscale, shift, out 16-byte aligned.  RMNET_E_UNSUPPORTED for another ksize / stride, Cout % 64 != 0, or
 * N*H*W*x_ld or N*Ho*Wo*out_ld >= 2^31; RMNET_E_INVALID_ARG for everything else.
 *
 * Weight pack (rmnet_amd.ops.flow_conv_pack), Cp = ceil32(Cin), e / ws / hi / lo / w_unscale as for rmnet_conv_split_f32:
 *   forward     w [Cout][Cin][k][k]:  fp16 [k*k][Cp / 32][2][Cout][32]: [tap = k * ky + kx][ci / 32][plane: hi, lo][co][ci % 32];
 *   transposed  w [Cin][Cout][4][4]:  fp16 [4][4][Cp / 32][2][Cout][32]: [phase = 2 * a + b][tap = 2 * ty + tx][ci / 32][plane][co][ci % 32]
 *               holding w[ci][co][3 - a - 2 * ty][3 - b - 2 * tx]; phase (a, b) computes the output pixels (2 i + a, 2 j + b) from the
 *               input pixels (i + a - 1 + ty, j + b - 1 + tx);
 *   both zero for ci >= Cin. */
#define RMNET_FLOW_RELU 1
#define RMNET_FLOW_LEAKY 2
#define RMNET_FLOW_TRANSPOSED 4
int rmnet_flow_conv_f32(const float *x, int x_ld, const void *wpack, const float *w_unscale, const float *shift, int flags, int N, int H,
                        int W, int Cin, int Cout, int ksize, int stride, float *out, int out_ld, int coff, int32_t *range_word,
                        void *stream);

/* C2 TinyFlowNet's flow heads (additive exports, same ABI version): out = conv3x3_p1(x[..., :Cin], w) + bias with two output channels
 * in plain fp32 FMA, straight from a channel-padded concatenation buffer (csrc/flow_head.hip).  Replaces predict_flow5 ..
 * predict_flow2 of TinyFlowNet (models/tiny_flownet.py) and the layout copy behind them.  No window and no range word.
 *   x     [N, H, W, x_ld] fp32 (channels-last), 16-byte aligned; x_ld % 4 == 0, x_ld >= Cin >= 1.  Channels Cin .. x_ld-1 are never
 *         used: any bit pattern, NaN included;
 *   wpack fp32 [ceil32(Cin)][9][2] (rmnet_amd.ops.flow_head_pack): w[co][c][ky][kx], unrounded, at (c * 9 + 3 * ky + kx) * 2 + co;
 *         zero for c >= Cin (ceil32: rounded up to a multiple of 32);
 *   bias  [2] fp32;  out [N, 2, H, W] fp32 NCHW;
 *   workspace: 16-byte aligned, at least rmnet_flow_head_workspace_bytes(N, H, W, Cin) bytes (0 for a non-positive size): the
 *         partial sums [ceil32(Cin) / 32][N][2][H][W] fp32 of the 32-channel slices.
 * Order of summation: the 32 channels of a slice per tap in channel order (FMA), the nine taps of a slice in the order ky, kx, then
 * bias + slice 0 + slice 1 + ...: fixed by Cin alone, no atomics -- the same bits from call to call and for any N.
 * RMNET_E_INVALID_ARG for a NULL pointer, a misaligned x or workspace, a workspace that is too small, and the size rules above;
 * RMNET_E_UNSUPPORTED for N*H*W*x_ld >= 2^31. */
size_t rmnet_flow_head_workspace_bytes(int N, int H, int W, int Cin);
int rmnet_flow_head_f32(const float *x, int x_ld, const float *wpack, const float *bias, int N, int H, int W, int Cin, float *out,
                        void *workspace, size_t workspace_bytes, void *stream);

/* C2 TinyFlowNet's flow upsamplers (additive export, same ABI version): ConvTranspose2d(2, 2, 4, stride 2, padding 1, no bias) of a
 * flow head's output, written into the next concatenation buffer in place (csrc/flow_head.hip).  Replaces upsampled_flow5_to_4 ..
 * upsampled_flow3_to_2 (models/tiny_flownet.py), the copy of their result into the buffer and the zero fill of its padding channels.
 *   flow  [N, 2, h, w] fp32 NCHW;  w [2][2][4][4] fp32: [ci][co][ky][kx], NCHW-contiguous;
 *   out   [N, 2h, 2w, out_ld] fp32 (channels-last), 16-byte aligned: channels coff, coff+1 of every pixel get the result, channels
 *         coff+2 .. out_ld-1 are set to +0.0, no other byte is written.  out_ld % 4 == 0, coff % 4 == 0, coff + 2 <= out_ld.
 * Output pixel (2i+a, 2j+b), channel co = sum over ci, ty, tx (in that order, FMA) of flow[ci][i+a-1+ty][j+b-1+tx] *
 * w[ci][co][3-a-2ty][3-b-2tx], taps outside the map skipped: the four phases of rmnet_flow_conv_f32.
 * RMNET_E_INVALID_ARG for a NULL pointer, a misaligned out and the size rules above; RMNET_E_UNSUPPORTED for N*2h*2w*out_ld >= 2^31. */
int rmnet_flow_up_f32(const float *flow, const float *w, int N, int h, int w_, float *out, int out_ld, int coff, void *stream);

/* P3/P4 tail: decoder logits -> foreground probability -> soft aggregation -> un-pad (-> soft-max over
 * the K mask channels) in one pass.  dec [n_tot,2,Hp,Wp]: 2-class logits of the objects in flight;
 * clip b owns objects [obj_begin[b], obj_begin[b+1]) (device int32 [B+1]); logit / prob [B,K,H,W] with
 * H,W the un-padded size and (pad_l, pad_t) the padding removed on the left / top.  prob may be NULL.
 * Replaces F.softmax(logit, dim=1)[:, 1], RMNet.soft_aggregation, the un-pad slicing and the per-frame
 * F.softmax of the frame loop: models/rmnet.py:368-380, 289-302, 450. */
int rmnet_soft_aggregate_f32(const float *dec, const int32_t *obj_begin, int B, int K, int Hp, int Wp,
                             int pad_l, int pad_t, int H, int W, float *logit, float *prob,
                             void *stream);

/* The gradient of that tail with respect to dec (additive export, same ABI version; csrc/soft_aggregate_bwd.hip), one streaming
 * pass: the backward of the soft-max over K (models/rmnet.py:450), of the edits of :436-448 (rmnet_object_edit_softmax_f32), of
 * the un-pad, of soft_aggregation and of F.softmax(dec, dim=1)[:, 1].  Per clip b with n = min(obj_begin[b+1] - obj_begin[b],
 * K - 1) objects and per output pixel, with p_o and bg the forward's fp32 values (re-created from dec by the forward's own code):
 *   s    = sum_k P_k g_k over all K channels, in channel order;   dl_k = P_k (g_k - s) + q_k
 *   live_k = k <= n and action[b][k] == 0;   pass(e) = 1e-7f <= e <= 1 - 1e-7f (ends inside as in torch.clamp, false for a NaN)
 *   a0   = live_0 and pass(bg) ? dl_0 / (1 - bg) : 0;   dz_o = (live_{o+1} and pass(p_o) ? dl_{o+1} : 0) - a0 p_o
 *   grad_dec[obj_begin[b] + o][1] = dz_o,  grad_dec[obj_begin[b] + o][0] = -dz_o          every operation rounded once, no FMA
 *   prob        P, the saved final probabilities [B,K,H,W] (after the edits on an edited frame), batch-strided like
 *               rmnet_object_edit_softmax_f32's: slice b starts at prob + b * prob_batch_stride and is contiguous
 *   grad_prob   g = d loss / d P, batch-strided likewise; may be NULL when grad_logit is given (then dl_k = q_k, P is not read)
 *   grad_logit  q = d loss / d logit (the logits after the edits), batch-strided likewise; may be NULL when grad_prob is given
 *   action      uint8 [B,K] as in rmnet_object_edit_softmax_f32 (0 keep, 1 absent, 2 inject), or NULL = every channel kept
 *   grad_dec    [n_tot,2,Hp,Wp]: EVERY element is written exactly once -- +0.0 in the padding rows and columns and for the objects
 *               o >= n of a clip with more than K - 1 objects -- so it needs no memset; no atomics, the same bits on every call.
 *               obj_begin[0] must be 0.
 * A NaN in dec makes P and therefore dl NaN at its pixel: every object of the clip whose channel or whose background passes gets a
 * NaN there, an object behind two masks gets 0, none gets a finite non-zero value.
 * Lane forms: 4 pixels per lane when Wp % 4 == 0 and dec, grad_dec are 16-byte aligned (prob / grad_prob / grad_logit are then read
 * with 16-byte loads too when W % 4 == 0, pad_l % 4 == 0, they are 16-byte aligned and their strides are multiples of 4), else 1.
 * RMNET_E_INVALID_ARG: a NULL dec, obj_begin, prob or grad_dec; grad_prob and grad_logit both NULL; a float pointer that is not
 * 4-byte aligned; B, K, H or W < 1; K > 255; pad_l or pad_t < 0; pad_l + W > Wp or pad_t + H > Hp; a given batch stride < K*H*W.
 * RMNET_E_UNSUPPORTED: B > 65535; 2*Hp*Wp, K*H*W, a stride or (B-1)*stride + K*H*W >= 2^31.  A refused call touches no buffer. */
int rmnet_soft_aggregate_bwd_f32(const float *dec, const int32_t *obj_begin, int B, int K, int Hp, int Wp, int pad_l, int pad_t, int H,
                                 int W, const float *prob, long long prob_batch_stride, const float *grad_prob,
                                 long long grad_prob_batch_stride, const float *grad_logit, long long grad_logit_batch_stride,
                                 const uint8_t *action, float *grad_dec, void *stream);

/* ---------------------------------------------------------------------------------------------
 * F1  Optical-flow update after two affine warps.
 * Replaces: CPython `flow_affine_transformation.update_optical_flow(flow, M1, M2)` --
 *           extensions/flow_affine_transformation/flow_affine_transformation.cpp:39-90.
 *   flow [H,W,2] f32, m1/m2 [2,3] f32 -> out [H,W,2] f32 (integer-valued).  Bit-exact with the
 *   reference's fp32 arithmetic (no FMA contraction, round-half-away-from-zero), including its
 *   quirk that y1 is computed from the already-updated x1 (.cpp:72-73).
 *   Alignment: flow and out 8-byte aligned (a pixel is read and written as one 8-byte access), m1 and m2 4-byte aligned;
 *   RMNET_E_INVALID_ARG otherwise, before any launch.
 * _host variant: all four pointers are HOST pointers (the reference's NumPy calling convention, any alignment a float
 * array has); it stages through `workspace` (device, >= rmnet_flow_affine_workspace_bytes, 8-byte aligned:
 * RMNET_E_INVALID_ARG otherwise, nothing copied) and synchronises the stream before returning.  Its staging pointers lie
 * at workspace, workspace + 256 and workspace + 256 + 8*H*W, so an 8-byte aligned workspace meets the rule above.
 * ------------------------------------------------------------------------------------------- */
int rmnet_flow_affine_f32(const float *flow, const float *m1, const float *m2, int H, int W,
                          float *out, void *stream);
size_t rmnet_flow_affine_workspace_bytes(int H, int W);
int rmnet_flow_affine_f32_host(const float *flow_host, const float *m1_host, const float *m2_host,
                               int H, int W, float *out_host, void *workspace,
                               size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * E1  Boundary measure F: the four integer counts per (frame, object) (additive exports, same ABI version).
 * Replaces: Metrics._get_f_score and Metrics.seg2bmap, utils/metrics.py:119-226, up to the counts -- the boundary maps of
 *           both masks, their dilation by skimage.morphology.disk(radius) and the sums of utils/metrics.py:147-152 -- for
 *           every object of every frame at once and without taking a label map off the device (csrc/boundary_f.hip).
 *           Precision, recall and F follow from the counts (utils/metrics.py:155-169: rmnet_amd.metrics.f_from_counts).
 *   pred, gt  [N,H,W] uint8 label maps, 0 = background; object k = (label == k) for k = 1 .. K, a label above K belongs
 *             to no object.
 *   radius    the disk's radius in pixels, ceil(0.008 * |(H, W)|) by the reference's rule (utils/metrics.py:134-135):
 *             8 at 480x854, 18 at 1080x1920, 36 at 2160x3840.  Offsets (dy, dx) with dx^2 + dy^2 <= radius^2; 0 = the
 *             centre tap alone.  The dilation reads 0 outside the image.
 *   counts    [N,K,4] int32 out: (n_fg, n_gt, fg_match, gt_match) = |bmap(pred_k)|, |bmap(gt_k)|,
 *             |bmap(pred_k) & dilate(bmap(gt_k))|, |bmap(gt_k) & dilate(bmap(pred_k))| with bmap = seg2bmap at the map's
 *             own size (utils/metrics.py:202-213).  Fully written (no pre-zeroing needed); exact integers, the same bits
 *             from call to call.
 *   workspace 8-byte aligned, at least rmnet_boundary_match_workspace_bytes(N, K, H, W) bytes (0 when any size is <= 0):
 *             the boundary maps as bit rows, [N][K][2][H][ceil(W/64)] 64-bit words.
 * RMNET_E_INVALID_ARG for a NULL pred / gt / counts, a non-positive size or a misaligned workspace; RMNET_E_UNSUPPORTED
 * for K > 64, radius < 0, radius > 40 or a launch of more than 2^31 - 1 workgroups (N*ceil(H/8)*ceil(W/64) / 4 or N*K*ceil(H*ceil(W/64) / 256));
 * RMNET_E_WORKSPACE for a NULL or short workspace.
 * ------------------------------------------------------------------------------------------- */
size_t rmnet_boundary_match_workspace_bytes(int N, int K, int H, int W);
int rmnet_boundary_match_u8(const uint8_t *pred, const uint8_t *gt, int N, int K, int H, int W, int radius, int32_t *counts,
                            void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * F1  Clip I/O: uint8 frames and label maps in, uint8 label maps and overlay frames out (additive exports, same ABI
 *     version; csrc/clip_io.hip).  Every result equals the reference's host arithmetic bit for bit.
 * Replaces: the loader's Normalize / ToOneHot after ReorganizeObjectID (utils/data_transforms.py:53-96 with
 *           img_normalize and to_onehot, utils/helpers.py:81-90, 133-135), torch.argmax over the probabilities and
 *           get_segmentation (core/inference.py:62-70, utils/helpers.py:138-178) up to the PNG encoder.
 * mean, std are HOST pointers to three doubles (the configuration's DATASET_MEAN / DATASET_STD); every other pointer is a
 * device pointer.  A lane owns 4 consecutive pixels (16 for the one-hot planes) when H*W and the pointers' alignment allow
 * dword / 16-byte accesses, and one pixel otherwise: any contiguous tensor is accepted.
 *
 * rmnet_frames_normalize_u8: frames [N,H,W,3] uint8 -> out [N,3,H,W] f32 with
 *     x = fl32(float(u) / 255.0f);  y = fl32((double(x) - mean[c]) / std[c])        (one rounding per operation)
 * rmnet_labels_onehot_u8: labels [N,H,W] uint8 -> out [N,K,H,W] uint8, out[n,k,y,x] = (lut[label] == k); lut is a device
 *     table of 256 uint8 or NULL for the identity.  A remapped label >= K sets no plane.  Fully written.
 *     ReorganizeObjectID's table: the ids present in the clip without the ignore id, ascending, map to 0, 1, 2, ...;
 *     every other id maps to 0 (rmnet_amd.clip_io.reorganize_lut builds it on the device).
 * rmnet_argmax_labels_f32: prob [N,K,H,W] f32 -> labels [N,H,W] uint8, the FIRST index of the maximum over K
 *     (torch.argmax's rule on ties).  1 <= K <= 255.  NaN inputs are out of scope: the inputs are soft-max outputs, and
 *     a NaN never compares greater, so it is passed over.
 * rmnet_overlay_u8: frames [N,3,H,W] f32 (the normalised frames the network consumed), labels [N,H,W] uint8
 *     -> out [N,H,W,3] uint8, per frame get_segmentation(frame, mask, {mean, std}, ignore_idx, alpha):
 *       denormalise   v_c = (uint8) trunc((double(x_c) * std[c] + mean[c]) * 255.0), three separately rounded operations
 *                     (this is not the source byte: some forty values per channel come back one lower).  Defined for
 *                     results in (-1, 256); saturates outside, NaN gives 0.
 *       S             the labels present in the frame, minus the smallest one present (np.unique(mask)[1:]: background
 *                     when there is any, otherwise the lowest object), minus ignore_idx.
 *       events        the pixel's own label L and the labels of its 4-neighbours inside the image, those in S, ascending:
 *                     o == L: v_c = (uint8) trunc(double(v_c) * alpha + (1.0 - alpha) * double(PALETTE[o][c]));
 *                     o != L: v = 0 (the pixel is on o's contour, binary_dilation(mask == o) ^ (mask == o)).
 *       PALETTE       the 16 DAVIS colours, then grey [i, i, i].  No product and sum is fused.
 *     workspace: int32 [N], 4-byte aligned, at least N * 4 bytes; the entry writes every frame's smallest label into it in
 *     two small launches ahead of the overlay launch (a fill with 255, then integer atomic minima).  It needs no
 *     initialisation by the caller, holds the same bits after every call and the three launches can be captured in a graph.
 *     An ignore_idx outside 0 .. 255 matches no label.
 * RMNET_E_INVALID_ARG for a NULL pointer (lut excepted), a non-positive size, alpha outside [0, 1], std[c] == 0 or a
 * pointer not aligned to its element type; RMNET_E_UNSUPPORTED for K > 255 or a launch of more than 2^31 - 1 workgroups
 * (N * ceil(H*W / 256) for one-pixel lanes); RMNET_E_WORKSPACE for a NULL or short workspace.
 * ------------------------------------------------------------------------------------------- */
int rmnet_frames_normalize_u8(const uint8_t *frames, int N, int H, int W, const double *mean, const double *std, float *out,
                              void *stream);
int rmnet_labels_onehot_u8(const uint8_t *labels, const uint8_t *lut, int N, int K, int H, int W, uint8_t *out, void *stream);
int rmnet_argmax_labels_f32(const float *prob, int N, int K, int H, int W, uint8_t *labels, void *stream);
int rmnet_overlay_u8(const float *frames, const uint8_t *labels, int N, int H, int W, const double *mean, const double *std,
                     double alpha, int ignore_idx, uint8_t *out, int32_t *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * H1  Multi-scale and flipped inference around the network passes (additive exports, same ABI version; csrc/tta.hip).
 * Replaces: the F.interpolate / torch.flip / torch.stack / torch.mean sequence of multi_scale_inference
 *           (utils/helpers.py:44-78) and the torch.argmax that follows it (core/inference.py:62).
 * Plain fp32, every product and sum rounded on its own.  The coordinate rule of one axis, axis(d, in, scale):
 *     s = max(fl(fl(scale * fl(d + 0.5f)) - 0.5f), 0);  i0 = min((int)s, in - 1);  i1 = min(i0 + 1, in - 1);
 *     l1 = fl(s - (float)i0);  l0 = fl(1 - l1)
 * and the value is  fl( fl(l0y * fl(fl(l0x*A) + fl(l1x*B))) + fl(l1y * fl(fl(l0x*C) + fl(l1x*D))) )  with A, B, C, D at
 * (i0y,i0x), (i0y,i1x), (i1y,i0x), (i1y,i1x): the formula torch's bilinear kernel is written from, align_corners=False.
 *
 * rmnet_resize_bilinear_f32: src [P,Hs,Ws] f32 -> dst [P,Hd,Wd] f32 with the scales as floats; for
 *     F.interpolate(scale_factor=fs) pass (float)(1.0 / fs) for both and Hd = floor(double(Hs) * fs), Wd likewise.
 *     flip != 0 writes column Wd - 1 - x: torch.flip(resized, dims=[-1]) in the same pass.  src and dst must not overlap.
 * rmnet_tta_merge_f32: E sources, srcs[e] a device pointer to [N,K,hs[e],ws[e]] f32; srcs, hs, ws, flipped are HOST arrays of
 *     E entries, copied into the launch.  Entry e is resized to (H, W) with the scales fl((float)hs[e] / (float)H) and
 *     fl((float)ws[e] / (float)W) (torch's rule for size=); a flipped entry is read at column ws[e] - 1 - x (the entry
 *     holds a mirrored clip).  acc = v_0, acc = fl(acc + v_e) in entry order, mean = fl(acc / (float)E), a true division.
 *     mean [N,K,H,W] f32 is fully written.  labels [N,H,W] uint8 (NULL: not wanted) is the first index of the maximum of the
 *     written means over K, byte for byte what rmnet_argmax_labels_f32 returns on mean.  No workspace, one launch.
 * RMNET_E_INVALID_ARG for a NULL pointer (labels excepted), a size < 1, E outside 1 .. RMNET_TTA_MAX_ENTRIES, K outside
 * 1 .. 255, a scale that is not finite and positive or a pointer not aligned to 4 bytes; RMNET_E_UNSUPPORTED for Hd or
 * ceil(H / 4) above 65535, a source side above 2^24 or a source plane of 2^31 elements or more.
 * ------------------------------------------------------------------------------------------- */
#define RMNET_TTA_MAX_ENTRIES 8
int rmnet_resize_bilinear_f32(const float *src, int P, int Hs, int Ws, int Hd, int Wd, float scale_h, float scale_w, int flip,
                              float *dst, void *stream);
int rmnet_tta_merge_f32(const float *const *srcs, const int *hs, const int *ws, const int *flipped, int E, int N, int K, int H,
                        int W, float *mean, uint8_t *labels, void *stream);

/* ---------------------------------------------------------------------------------------------
 * I1  Objects that are first annotated in the middle of a clip, the YouTube-VOS protocol (additive exports, same ABI version;
 *     csrc/late_objects.hip).
 * Replaces: the np.unique of every label map behind the loader's cumulative object count (utils/data_loaders.py:58-65) and
 *           behind existing_objects (models/rmnet.py:398-407, 438), and the per-frame index writes of models/rmnet.py:436-448
 *           with the F.softmax of :450, without one-hot masks of any frame but the first.
 *
 * rmnet_label_presence_u8: labels [N,H,W] uint8 at ANY byte alignment -> presence [N,8] uint32: bit (v & 31) of word (v >> 5) of
 *     row n is set exactly when byte value v occurs in frame n.  The entry zeroes presence on the stream ahead of its one launch
 *     (a memset node under graph capture), so the caller initialises nothing.  A frame is read as a head of up to 15 bytes in
 *     front of the first 16-byte boundary, 16-byte loads, and a tail of up to 15 bytes; rmnet_label_presence_chunk_bytes() is
 *     the number of body bytes one workgroup takes (pure host arithmetic).  The words are OR-ed together with integer atomics,
 *     which commute: the same bits after every call.  No LDS, no workspace.
 * RMNET_E_INVALID_ARG for a NULL pointer, N, H or W < 1 or a presence that is not 4-byte aligned; RMNET_E_UNSUPPORTED for
 * N*H*W >= 2^31.
 *
 * rmnet_object_edit_softmax_f32: one frame of models/rmnet.py:436-450 in one pass.
 *     logit  f32 [B,K,H,W], slice b at logit + b * logit_batch_stride (elements); EDITED IN PLACE
 *     labels uint8 [B,H,W], slice b at labels + b * labels_batch_stride: frame t's raw label maps; NULL when no action is 2
 *            (an action 2 without a label map injects m = 0 everywhere)
 *     lut    uint8 [B,256]: ReorganizeObjectID's table of every clip (see rmnet_labels_onehot_u8)
 *     action uint8 [B,K] on the device: 0 (and every value above 2) keeps the channel, 1 marks it absent, 2 injects
 *     prob   f32 [B,K,H,W], slice b at prob + b * prob_batch_stride: fully written; with the stride it may be est[:, t] of a
 *            [B,N,K,H,W] tensor.  Must not overlap logit.
 *   absent  l = -16.1181f
 *   inject  l = fl(fl(m * 32.0605f) - 16.1181f), m = (lut[b][label] == k) as 1.0f / 0.0f: fp32, one rounding per operation, as
 *           torch evaluates masks.float() * 32.0605 - 16.1181
 *   keep    the stored bits are neither touched nor rewritten
 *   soft-max  mx = l_0, mx = fmaxf(mx, l_k) for k ascending;  sum = e_0, sum = fl(sum + e_k) for k ascending with
 *           e_k = expf(fl(l_k - mx));  p_k = fl(e_k / sum), a true division.  expf is the device library's, the one
 *           rmnet_soft_aggregate_f32 calls.
 *     1 <= K <= 255.  NaN logits are out of scope: fmaxf passes over a NaN, so the pixel's other channels would be
 *     normalised as if it were not there while its own probability is a NaN.
 *     A lane owns 4 consecutive pixels when H*W, both strides and both float pointers allow 16-byte accesses, else one.
 * RMNET_E_INVALID_ARG for a NULL pointer other than labels, B, H or W < 1, K outside 1 .. 255, a float pointer not aligned to
 * 4 bytes or a batch stride smaller than the slice it steps over (K*H*W; H*W for labels); RMNET_E_UNSUPPORTED for B > 65535
 * or an element index (a stride, K*H*W, or (B - 1) * stride + slice) of 2^31 or more.
 * ------------------------------------------------------------------------------------------- */
int rmnet_label_presence_chunk_bytes(void);
int rmnet_label_presence_u8(const uint8_t *labels, int N, int H, int W, uint32_t *presence, void *stream);
int rmnet_object_edit_softmax_f32(float *logit, long long logit_batch_stride, const uint8_t *labels, long long labels_batch_stride,
                                  const uint8_t *lut, const uint8_t *action, float *prob, long long prob_batch_stride, int B, int K,
                                  int H, int W, void *stream);

/* ---------------------------------------------------------------------------------------------
 * I2  I1 for a clip that runs at another scale, possibly mirrored: late objects under multi-scale and flipped inference
 *     (additive exports, same ABI version; csrc/late_objects.hip).
 * Replaces: F.interpolate(masks, scale_factor=fs, mode='nearest') and torch.flip of the one-hot masks of EVERY frame in
 *           multi_scale_inference (utils/helpers.py:44-78) as far as models/rmnet.py:398-407, 436-450 read them: the
 *           torch.unique(torch.argmax(masks[t])) of frame 0 and of every frame with new objects, and the injected plane.
 * The sampling rule of one axis, for output index d of an axis with `in` source elements:
 *     src(d) = min((int)floorf((float)d * scale), in - 1)
 * with scale = (float)(1.0 / fs) for F.interpolate(scale_factor=fs) and the output size floor(double(in) * fs): torch's legacy
 * 'nearest' mode as a plain formula.  (torch's own kernels copy an axis whose output size equals its input size or its double
 * even when fs is neither 1 nor 2; this rule does not.)  Nearest-resizing one-hot planes and taking their argmax equals applying
 * the clip's table to the sampled label, so nothing but the full-size label maps is read and no resized map is written.
 *
 * rmnet_label_presence_nearest_u8: labels [N,Hs,Ws] uint8 at ANY byte alignment and S scales -> presence [S,N,8] uint32: bit
 *     (v & 31) of word (v >> 5) of row (s, n) is set exactly when v occurs among labels[n][src_h(y)][src_w(x)] for y < hd[s],
 *     x < wd[s].  hd, wd, scale_h, scale_w are HOST arrays of S entries, copied into the launch.  All scales are covered by one
 *     launch behind the memset the entry issues itself (a memset node under graph capture); integer atomics, the same bits
 *     after every call; no LDS, no workspace.  rmnet_label_presence_nearest_rows() is the number of output rows of one scale
 *     that one workgroup takes (pure host arithmetic).
 * RMNET_E_INVALID_ARG for a NULL pointer, N, Hs, Ws, hd[s] or wd[s] < 1, S outside 1 .. RMNET_TTA_MAX_ENTRIES, a scale that is
 * not finite and positive or a presence that is not 4-byte aligned; RMNET_E_UNSUPPORTED for a side above 2^24 (the float index
 * must be exact) or N*Hs*Ws >= 2^31.
 *
 * rmnet_object_edit_softmax_nearest_f32: rmnet_object_edit_softmax_f32 on a frame of H x W whose labels are read from a
 *     full-size map: labels uint8 [B,Hs,Ws], slice b at labels + b * labels_batch_stride, and pixel (y, x) of slot b takes
 *     labels[b][src_h(y)][src_w(xx)] with xx = W - 1 - x when bit b of flip_bits is set (the slot holds a mirrored clip), else
 *     x.  labels_batch_stride may be 0: every slot reads the same map (a clip and its mirrored twin; the maps are only read).
 *     Everything else -- constants, walks, rounding, lane forms, strides -- is rmnet_object_edit_softmax_f32's: on a
 *     materialised resized (and mirrored) label map that entry returns the same bits in logit and in prob.
 * The refusals of rmnet_object_edit_softmax_f32, with H*W of labels replaced by Hs*Ws, and: RMNET_E_INVALID_ARG for Hs or
 * Ws < 1 or a scale that is not finite and positive; RMNET_E_UNSUPPORTED for B > 64 (one flip bit per slot) or a side above 2^24.
 * ------------------------------------------------------------------------------------------- */
int rmnet_label_presence_nearest_rows(void);
int rmnet_label_presence_nearest_u8(const uint8_t *labels, int N, int Hs, int Ws, const int *hd, const int *wd,
                                    const float *scale_h, const float *scale_w, int S, uint32_t *presence, void *stream);
int rmnet_object_edit_softmax_nearest_f32(float *logit, long long logit_batch_stride, const uint8_t *labels,
                                          long long labels_batch_stride, int Hs, int Ws, float scale_h, float scale_w,
                                          unsigned long long flip_bits, const uint8_t *lut, const uint8_t *action, float *prob,
                                          long long prob_batch_stride, int B, int K, int H, int W, void *stream);

/* ---------------------------------------------------------------------------------------------
 * I1  Validation loss of a clip: Lovasz-softmax brackets and the NLL sum (additive exports, same ABI version;
 *     csrc/val_loss.hip).
 * Replaces: lovasz_loss(est_probs, masks) + nll_loss(torch.log(est_probs), masks) of core/test.py:97 (models/lovasz_loss.py
 *           and torch.nn.NLLLoss), without the reference's permuting copy, its sort of all pixels per class and its fp32 cumsums.
 *   probs        [N,K,H,W] float32, 4-byte aligned (any alignment beyond that); labels [N,H,W] uint8 at any byte alignment.
 *   ignore_index a label value 0 .. 255 whose pixels are left out; any other value: nothing is ignored.
 *   bins         a power of two, 2 .. 2^22.
 *   A pixel that is not ignored is BAD when its label is >= K (checked first) or when any of its K probabilities is not
 *   inside [0, 1] (NaN included); bad pixels are counted and left out of everything.  For every other pixel and every class c:
 *   fg = (label == c), e = fabsf((float)fg - p_c), key = (unsigned)(e * (float)bins) in [0, bins] (bin `bins` holds e == 1
 *   alone), hist[c][fg][key] += 1, and nll_sum += -logf(p_label) in float64 (+inf for p_label == 0).
 *   per_class    [K][3] double out: G = the class's foreground count, lo, hi with, in float64 and Fge / Bge (Fgt / Bgt) the
 *                sums of hist[c][1] / hist[c][0] over the bins >= k (> k),
 *                  hi = (1/bins) sum_{k=0}^{bins-1} 1 - (G - Fge(k)) / (G + Bge(k)),   lo = the same with Fgt, Bgt.
 *                lo <= the class's Lovasz extension <= hi and hi - lo <= 1/bins.  lo = hi = 0 when G == 0.
 *   nll_sum      [1] double out;  counts [3] long long out: good pixels, bad by label, bad by probability.
 *   workspace    8-byte aligned, at least rmnet_clip_loss_workspace_bytes(K, bins) bytes (0 when K is outside 1 .. 255 or bins
 *                is no power of two in range).  It begins with hist, uint32 [K][2][bins + 1] (index 0 = background,
 *                1 = foreground), complete when the call's work is; the per-workgroup partials follow.  The call clears what it
 *                accumulates into; every output is fully written.  Counts are exact integers and every float64 sum has a fixed
 *                order: the same bits from call to call.
 * RMNET_E_INVALID_ARG for a NULL pointer, a non-positive size, K outside 1 .. 255, a bad `bins` or a misaligned pointer;
 * RMNET_E_UNSUPPORTED for N*H*W >= 2^31; RMNET_E_WORKSPACE for a NULL or short workspace.  Nothing is launched then.
 * ------------------------------------------------------------------------------------------- */
size_t rmnet_clip_loss_workspace_bytes(int K, int bins);
int rmnet_clip_loss_f32(const float *probs, const uint8_t *labels, int N, int K, int H, int W, int ignore_index, int bins,
                        double *per_class, double *nll_sum, long long *counts, void *workspace, size_t workspace_bytes,
                        void *stream);

/* ---------------------------------------------------------------------------------------------
 * I2  Training loss of a clip, value and gradient: everything I1 returns and d(lovasz + nll) / d probs (additive exports, same
 *     ABI version; csrc/val_loss_bwd.hip).
 * Replaces: loss = lovasz_loss(est_probs, masks) + nll_loss(torch.log(est_probs), masks); loss.backward() of core/train.py:180,
 *           as far as est_probs: no permuted copy, no sort, no int64 permutation, no index-scatter backward.
 *   probs, labels, ignore_index, bins, per_class, nll_sum, counts: as in I1, and with the same bits as I1 returns.
 *   grad         [N,K,H,W] float32 out, 4-byte aligned, not overlapping probs.  With key as in I1, G the class's foreground
 *                count, F> / B> the sums of hist[c][1] / hist[c][0] over the bins above key and F>= / B>= those over the bins at or
 *                above it, in float64 and rounded once to float32:
 *                  g_fg[c][key] = (1 / (G + B>) + 1 / (G + B>=)) / 2
 *                  g_bg[c][key] = (G - (F> + F>=) / 2) / ((G + B>) (G + B>=))               (both 0 for a class with G == 0)
 *                and, in fp32 with one rounding per operation, s = -1 on a foreground element, +1 on a background one, 0 where
 *                e == 0, n_present the classes with G > 0 and n_good = counts[0]:
 *                  grad = (s * g) * (float)(1.0 / n_present)   [+ (float)(-1.0 / ((double)p * (double)n_good)) where c == label]
 *                (-inf where p_label == 0).  All K elements of an ignored or bad pixel are 0.  This is the subgradient of the
 *                Lovasz extension at the errors quantised to their bins: the mean of the two orders "the bin's foregrounds first"
 *                and "the bin's backgrounds first"; it is the gradient of the reference's sort exactly where no bin of a class
 *                holds more than one pixel, and within the span of the sort's possible tie orders everywhere.
 *                Every element is written exactly once (the caller never pre-zeros); no atomics: the same bits from call to call.
 *   workspace    8-byte aligned, at least rmnet_clip_loss_grad_workspace_bytes(K, bins) bytes.  When the call's work is complete
 *                it begins with the tables, float32 [K][2][bins + 1] (index 0 = g_bg, 1 = g_fg), in the place of I1's hist.
 * The refusals of I1, and RMNET_E_INVALID_ARG for a NULL or misaligned grad or one that overlaps probs.  Nothing is launched then.
 * ------------------------------------------------------------------------------------------- */
size_t rmnet_clip_loss_grad_workspace_bytes(int K, int bins);
int rmnet_clip_loss_grad_f32(const float *probs, const uint8_t *labels, int N, int K, int H, int W, int ignore_index, int bins,
                             float *grad, double *per_class, double *nll_sum, long long *counts, void *workspace,
                             size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * J1  Adjoint of the bilinear upsample by 2 or 4, align_corners = False (additive exports, same ABI version;
 *     csrc/decoder_glue_bwd.hip).
 * Replaces: the backward of F.interpolate(x, scale_factor=S, mode='bilinear', align_corners=False) (models/rmnet.py:117-119, 139),
 *           which scatters with floating-point atomic adds on the GPU.
 *   g    [N,C,S h,S w] float32, the gradient of the fine map;  out [N,C,h,w] float32, every element written exactly once.
 *        nhwc != 0: both are [N,.,.,C] in memory, C % 4 == 0, both 16-byte aligned; otherwise NCHW, 4-byte aligned (fine rows are
 *        read 16 bytes at a time when g is 16-byte aligned and S w % 4 == 0).  out must not overlap g.
 *   With the forward's rule src = max((d + 0.5) / S - 0.5, 0), i0 = floor(src), i1 = i0 + (i0 < n - 1), coarse j of an axis of length n
 *   reads the fine indices S j - S/2 + t, t = 0 .. 2 S - 1, with the weights (2 t + 1) / (2 S) for t < S and their mirror image behind;
 *   at j = 0 the first S/2 taps do not exist and the next S/2 weigh 1; at j = n - 1 the mirror image of that.  2-D is the outer
 *   product.  Order of one element: fine rows ascending; in a row s = fma(wx, g, s) over the existing fine columns ascending from
 *   s = 0, then acc = fma(wy, s, acc).  No atomics: the same bits from call to call.
 * RMNET_E_INVALID_ARG for a NULL or misaligned pointer, a non-positive size, C % 4 under nhwc or overlapping buffers;
 * RMNET_E_UNSUPPORTED for any other factor or >= 2^31 elements of g.  Nothing is launched then.
 * ------------------------------------------------------------------------------------------- */
int rmnet_upsample_bwd_f32(const float *g, long long N, int C, int h, int w, int factor, int nhwc, float *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * J2  Backward of the prediction head (rmnet_pred_head_f32), out = conv3x3_p1(relu(x), w) + bias (additive exports; csrc/decoder_glue_bwd.hip).
 * Replaces: the backward of self.pred2(F.relu(m2)) (models/rmnet.py:138): threshold_backward, the library's two convolution
 *           gradients and the layout copies between them.
 *   x  [n,Hq,Wq,C] float32 channels-last, C % 32 == 0, 16-byte aligned;  w [2][C][3][3], 16-byte aligned;  g [n,2,Hq,Wq] NCHW.
 *   With G[k][ky][kx](y, x) = g[k][y - ky + 1][x - kx + 1], zero outside the map:
 *   dx [n,Hq,Wq,C] channels-last, 16-byte aligned:  [x > 0] * sum over k, ky, kx (that order, fma from 0) of w[k][c][ky][kx] * G;
 *                  a NaN in x gives 0 (threshold_backward's rule).
 *   dw [2][C][3][3]:  sum over the pixels of relu(x)[p][c] * G[k][ky][kx](p), relu(x) = x > 0 ? x : 0 (a NaN counts as 0).
 *   db [2]:           sum over the pixels of g[k][p].
 *   Any of dx, dw, db may be NULL: that part is skipped (all three: nothing is launched, RMNET_OK).  dw and db are summed per pixel
 *   range (32 slots of every 32nd pixel, added in slot order) into the workspace and merged in range order by a second kernel: no
 *   atomics, every element written once, the same bits from call to call.
 *   workspace  16-byte aligned, at least rmnet_pred_head_bwd_workspace_bytes(n, Hq, Wq, C) bytes (0 for a shape that is refused);
 *              only read when dw or db is asked for.
 * RMNET_E_INVALID_ARG for a NULL x / w / g, a non-positive size, a misaligned pointer, or an output that overlaps an input or
 * another output; RMNET_E_UNSUPPORTED for C % 32 != 0 or n Hq Wq C >= 2^31; RMNET_E_WORKSPACE for a NULL or short workspace when dw
 * or db is asked for.  Nothing is launched then.
 * ------------------------------------------------------------------------------------------- */
size_t rmnet_pred_head_bwd_workspace_bytes(int n, int Hq, int Wq, int C);
int rmnet_pred_head_bwd_f32(const float *x, const float *w, const float *g, int n, int Hq, int Wq, int C, float *dx, float *dw,
                            float *db, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RMNET_HIP_H_ */
