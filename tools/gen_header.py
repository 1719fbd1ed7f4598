#!/usr/bin/env python
"""Regenerate include/jperceiver_hip.h from the extern "C" definitions in jperceiver_amd/csrc.
The per-function notes (which reference interface each entry point replaces) live here."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = "mono/model/mono_baseline/"
GROUPS = [
    ("Convolution (fp32 MFMA implicit GEMM) — replaces nn.Conv2d / ReflectionPad2d+Conv2d: "
     + R + "resnet.py:6-13,91; " + R + "layers.py:147-167; " + R + "depth_decoder.py:15-39; " + R + "pose_decoder.py:9-12; "
     + R + "layout_model.py:31-47,138-153; " + R + "CrossViewTransformer.py:30-42.  *_src3: the input is the channel concat of up to 3 "
     "tensors, each optionally stored at half resolution (fused F.interpolate(scale_factor=2,'nearest') + torch.cat, "
     + R + "depth_decoder.py:68,76-77).  pad_mode 0=zero 1=reflect; act 0=none 1=relu 2=leaky_relu(0.01) 3=sigmoid.  ws / ws_state: caller scratch for the packed weights "
     "(jp_conv2d_ws_floats) and whether it already holds this layer's pack (1) or must be packed by this call (0); packs recorded with "
     "jp_pack_record_begin/end can be refreshed for the whole model by one jp_pack_replay launch per step (job table in device memory; every job's `begin` is the running sum of the totals rounded up to a multiple of 4, "
     "total_elems the rounded grand total: the replay kernel works on groups of 4 consecutive elements; generic_elems: where the jobs of the "
     "LDS-staged split-pack kernel -- jp_pack_mode_is_split(job.mode) -- begin when the caller put them at the tail of the table, 0 = not sorted).  "
     "bn_stats / bn_stats_parts (forward): optional scratch of jp_conv2d_fwd_bn_stats_floats floats for a convolution that feeds a train-mode "
     "BatchNorm (" + R + "resnet.py:29-45; no bias, no activation): the 4-wave 3x3 patch kernels leave per-channel partial sums of y and y^2 "
     "there and *bn_stats_parts (host int) = the partials per channel, to be handed to jp_bn_train_fwd (conv_stats / conv_parts) in place of "
     "its own statistics pass over y; 0 = the kernel that ran the layer does not (NULL: not wanted).  "
     "ARITHMETIC: fp32 in / out / accumulate.  The patch kernels (3x3, 1x1, 7x7 stem, iconv; JP_P9S / JP_W9S / JP_P9US / JP_P9SD / JP_P9S2 / JP_P7S, default on) "
     "form each fp32 product on the 16-bit matrix pipe.  Default build (JP_NS = 2, jp_split_scheme() == 2): 3 fp16 products a0 b0 + a0 b1 + a1 b0 "
     "of two-way fp16 splits of both operands, each operand TENSOR scaled by the power of two that puts its largest magnitude into "
     "[2^14, 2^15) (csrc/igemm_p9s.h:jp_split2h, csrc/scale.hip; magnitudes: the jp_amax* group below).  Operands are carried to 2^-23 "
     "relative for elements within 2^-17 of their tensor's largest, to 2^-40 OF THAT LARGEST below; the term left out is <= 2^-22 |a b|.  "
     "Measured against float64 on layer data the rms error is 0.62-1.00 x the exact-fp32 MFMA kernels' (profiles/r05_fp16x2_accuracy_vs_f64.md; "
     "tests/test_split_accuracy_gpu.py holds it to 1.25 x and every output to 2^-19 sum|a||b|; tools/split_study.py: the split error is 3-4 x "
     "below the fp32 accumulation's own rounding).  It is an error relative to the tensor's largest magnitude, not to each element: outputs "
     "that depend only on values > 2^29 below their tensor's largest lose relative precision.  MEASURED LIMITS on the GPU kernels "
     "(tests/test_split_accuracy_gpu.py::test_split_accuracy_where_one_scale_per_tensor_differs_from_fp32, profiles/r06_split_outliers.md; "
     "8 x 128 -> 128 3x3 @64^2 next to the exact-fp32 kernels): one activation 10^6 x the median costs the outputs that do NOT read it 1.6 x "
     "(forward) / 2.7 x (weight gradient) the rms error of the fp32 accumulation; a channel whose data all sits 2^20 below its tensor's "
     "largest has ITS weight gradients carried to 7e-6 relative rms (fp32: 3e-7); log-normal gradients (sigma 3 / 4), 10^4 outliers, a "
     "filter 2^12 above the rest: no further from float64 than the exact-fp32 kernels.  RANGE EDGES "
     "(test_split_range_edges_match_documented_behaviour): Inf / NaN inputs and finite ones with |x| >= 2^100 take no part in the scale and "
     "make exactly the outputs that read them NaN (an fp32 convolution yields +-Inf for an Inf input); everything else is bit-identical to "
     "the run without them.  Tensors of tiny values are lifted by their scale (2^-120 inputs: full accuracy).  The 7x7 stem and the stride-2 "
     "weight gradient (JP_P7S, W9S2) and a -DJP_NS=3 build use 6 bf16 products of exact 3-way bf16 splits (csrc/igemm_p9s.h:jp_split3: error "
     "<= the fp32 FMA chain's for 2^-109 <= |x| <= 3.3895e38; Inf -> NaN).  JP_P9S=0 JP_W9S=0 JP_P9US=0 JP_P9SD=0 JP_P9S2=0 selects the "
     "exact-fp32 MFMA kernels, which have none of these edges.",
     ["jp_conv2d_fwd", "jp_conv2d_fwd_src3", "jp_conv2d_dgrad", "jp_conv2d_dgrad_src3", "jp_conv2d_dgrad_src3_split_floats", "jp_conv2d_dgrad_src3_ok", "jp_conv2d_up_head_ok", "jp_conv2d_wgrad", "jp_conv2d_wgrad_src3", "jp_conv2d_ws_floats", "jp_conv2d_fwd_bn_stats_floats", "jp_conv2d_fwd_split_floats", "jp_conv2d_dgrad_split_floats", "jp_conv2d_wgrad_ws_floats", "jp_conv2d_wgrad_src3_ws_floats", "jp_channel_sum_ws_floats", "jp_channel_sum", "jp_pack_job_bytes", "jp_pack_record_begin", "jp_pack_record_end", "jp_pack_mode_is_split", "jp_pack_replay"]),
    ("Operand scales of the fp16 split kernels (csrc/scale.hip, csrc/igemm_p9s.h:jp_split2h) -- no counterpart in the reference: plumbing of "
     "the arithmetic above, and since ABI version 3 entirely in the entry points' own ARGUMENTS (no library-owned device memory, no state "
     "between calls).  A kernel that forms its fp32 products from two fp16 splits per operand reads the operand tensor's largest "
     "magnitude from device memory.  A magnitude lives in a SLOT of jp_amax_slot_floats() floats (512: 32 words one cache line apart -- "
     "producers spread their atomics over them, the kernels take the maximum; every `amax_*` / `out` argument is one).  "
     "INPUT magnitudes -- amax_x / amax_x0..2 (forward, weight gradient), amax_dy (dgrad, weight gradient) of the jp_conv2d_* entry points: "
     "a slot that holds max |operand| on `stream` (from jp_amax, or written by the producer of the tensor, below), or NULL; for every "
     "operand passed as NULL the call reduces the tensor itself (one extra read) into `amax_ws`, caller scratch of "
     "jp_conv2d_amax_ws_floats() floats that need not be initialised and may be reused by the next call on the same stream.  A call with "
     "a NULL operand magnitude AND amax_ws == NULL is a bad argument, and so is a forward call with more than one source and no amax_ws "
     "(its kernel reads ONE magnitude, the largest of the sources', folded into the scratch by a 64-lane launch); the -DJP_NS=3 build "
     "ignores all of them.  A magnitude that is too "
     "SMALL overflows fp16 (Inf / NaN outputs); one that is too large only costs precision (an upper bound is enough: max-pool and ReLU "
     "outputs may reuse their input's slot).  "
     "OUTPUT magnitudes -- a producer folds max |tensor it writes| into the slot with atomic maxima (the slot must hold 0, or an earlier "
     "maximum to extend): jp_bn_train_fwd / jp_bn_relu_pool_fwd amax_y, jp_sum_n amax_out, jp_bn_train_bwd / jp_act_bwd / jp_act_bwd_bias / "
     "jp_maxpool_bwd amax_dx (NULL: not wanted), and the convolutions -- jp_conv2d_fwd* amax_y, jp_conv2d_dgrad amax_dx, "
     "jp_conv2d_dgrad_src3 amax_dx0 (the first source's gradient): folded in by the kernel's epilogue (and, for the backward of "
     "reflection-padded layers, by the border fold) when a patch kernel runs the layer, in which case *amax_y_done / *amax_dx_done "
     "(host int, may be NULL) is set to 1 before the call returns; 0 = the kernel chosen for this shape does not report "
     "(use jp_amax on the tensor if the magnitude is needed).  "
     "jp_amax writes max |x[0..n)| (Inf / NaN / |x| >= 2^100 excluded) to *out (jp_amax_into: max(*out, that) -- *out pre-zeroed by the "
     "caller, no memset).  jp_split_scheme: 2 = this build's patch kernels use the fp16 two-way split (magnitudes are read), 3 = the "
     "bf16 three-way split (no operand scales).",
     ["jp_amax_slot_floats", "jp_conv2d_amax_ws_floats", "jp_amax", "jp_amax_into", "jp_split_scheme"]),
    ("Train-mode BatchNorm2d (+fused residual add / ReLU) — " + R + "resnet.py:21-24,41-45,92; " + R + "layout_model.py:146,152. "
     "ws = jp_bn_ws_doubles(N, C, HW) doubles of caller scratch.  n_updates = number of momentum updates of the running stats (2 for the layout "
     "branch the reference evaluates twice, " + R + "net.py:73-74).  jp_bn_relu_pool_*: the ResNet stem tail bn1 -> relu -> MaxPool2d(3, 2, 1) ("
     + R + "resnet.py:92-94) in one pass each way, for callers that do not read the normalised map itself (the decoders never do): "
     "pooled output + argmax byte in forward, the convolution-output gradient straight from the pooled gradient in backward.",
     ["jp_bn_ws_doubles", "jp_bn_train_fwd", "jp_bn_train_bwd", "jp_bn_eval_fwd", "jp_bn_relu_pool_fwd",
      "jp_bn_relu_pool_bwd_ws_doubles", "jp_bn_relu_pool_bwd"]),
    ("Frozen inference (csrc/frozen.hip; model/modules.py FrozenConvBN, apis.freeze) -- an eval-mode BatchNorm2d behind a convolution ("
     + R + "resnet.py:29-45,92; " + R + "layout_model.py:138-153) folded into that convolution, no counterpart in the reference.  "
     "jp_bn_fold_conv: w (Cout, K) with K = Cin*KH*KW, conv_bias (Cout) or NULL (= 0); per output channel in float64 "
     "s = gamma / sqrt(running_var + eps), w_out[c,:] = float(w[c,:] * s), bias_out[c] = float(beta + (conv_bias - running_mean) * s), "
     "each operation rounded once and nothing clamped (negative, zero and tiny gamma come out as the formula says); one workgroup per "
     "channel; w_out != w.  Run once per freeze, then the folded pair is jp_conv2d_fwd* with bias and act.  jp_add_relu: out = a + b, "
     "then max(., 0) when relu != 0 -- the tail of a BasicBlock after folding (residual add + ReLU), one pass, 16-byte accesses when the "
     "three pointers are 16-byte aligned and a scalar tail; out may be a (not b).  The ReLU is `r > 0 ? r : 0`, the result of "
     "jp_bn_eval_fwd's fmaxf(r, 0) which it replaces: a NaN sum becomes 0 (torch.relu would keep the NaN) and -0.0 becomes +0.0; "
     "with relu == 0 the sum is stored as it is, NaN included (max |out| ignores a NaN either way).  amax_out: optional magnitude slot that receives "
     "max |out| (the convention of jp_sum_n amax_out above).",
     ["jp_bn_fold_conv", "jp_add_relu"]),
    ("Pooling / resampling / elementwise — MaxPool2d " + R + "resnet.py:94, " + R + "layers.py:191, " + R + "layout_model.py:84; "
     "nearest upsample " + R + "layers.py:110; torch.cat; Dropout multiply " + R + "depth_decoder.py:52-53; F.interpolate bilinear "
     + R + "net.py:196,632,692 and area " + R + "net.py:762.",
     ["jp_maxpool_fwd", "jp_maxpool_bwd", "jp_upsample2x_fwd", "jp_upsample2x_bwd", "jp_copy_channels", "jp_axpby", "jp_sum_n", "jp_mul",
      "jp_affine", "jp_act_fwd", "jp_act_bwd", "jp_act_bwd_bias_ws_floats", "jp_act_bwd_bias", "jp_mul_bcast_c", "jp_mul_bcast_c_bwd_s", "jp_bilinear_fwd", "jp_bilinear_bwd",
      "jp_area_downsample", "jp_fill", "jp_warp_perspective", "jp_softmax_c2", "jp_disp_to_depth",
      "jp_scale_label_assemble", "jp_fill_convex_poly"]),
    ("Small dense algebra of the BEV branch — CVP MLP " + R + "CycledViewProjection.py:33-38,54-67; CCT attention "
     + R + "CrossViewTransformer.py:14-24,53-65,77-88; PoseDecoder spatial mean " + R + "pose_decoder.py:22-23.",
     ["jp_gemm_strided_batched", "jp_bias_act_rows", "jp_colsum", "jp_colmax", "jp_colmax_bwd", "jp_gather_cols",
      "jp_gather_cols_bwd", "jp_spatial_mean", "jp_spatial_mean_bwd", "jp_bcast_matmul_fwd", "jp_bcast_matmul_bwd",
      "jp_ratio_finalize"]),
    ("CGT view synthesis + photometric losses — pose " + R + "net.py:704-756; Backproject/Project/grid_sample "
     + R + "layers.py:41-82, " + R + "net.py:690-702; SSIM " + R + "layers.py:85-107; reprojection + automask min "
     + R + "net.py:84-92,159-175.",
     ["jp_pose_fwd", "jp_pose_bwd", "jp_cgt_warp_fwd", "jp_cgt_warp_bwd", "jp_ssim_l1_fwd", "jp_ssim_l1_bwd",
      "jp_minreproj_fwd", "jp_scalar_finalize", "jp_ssim_map", "jp_backproject", "jp_project"]),
    ("Other losses — smoothness " + R + "net.py:182-190,758-786; CGT scale loss " + R + "net.py:193-211; IoU "
     + R + "dice_loss.py:31-81,293-331 + weighted CE " + R + "net.py:561,583 + boundary loss " + R + "boundary_loss.py:121-192 "
     "(jp_sdf = exact EDT + inner boundary on the GPU, no host round trip); cycle L1 " + R + "net.py:619-622.",
     ["jp_row_sum", "jp_smooth_fwd", "jp_smooth_bwd", "jp_scale_loss_fwd", "jp_scale_loss_bwd", "jp_layout_loss_fwd",
      "jp_layout_loss_bwd", "jp_sdf", "jp_l1_fwd", "jp_l1_bwd"]),
    ("Optimizer over flat arenas + RNG — clip_grads(max_norm=35)+Adam mono/core/utils/dist_utils.py:58-60, "
     "config/cfg_kitti_baseline_odometry_boundary_ce_iou_1024_20.py:69-70; Dropout / randn " + R + "depth_decoder.py:13, "
     + R + "net.py:163.",
     ["jp_sumsq_blocks", "jp_grad_sumsq_partials", "jp_sum_doubles", "jp_adam_clip_step", "jp_adam_clip_step_dev", "jp_rng_keep_mask",
      "jp_rng_normal", "jp_rng_keep_mask_dev", "jp_rng_normal_dev"]),
    ("Evaluation metrics as GPU reductions — mean_IU / mean_precision mono/core/evaluation/pixel_error.py:59-118 (confusion counts "
     "of argmax(logits) vs label); depth compute_errors + median scaling + Garg crop mono/core/evaluation/pixel_error.py:27-40, "
     "mono/core/evaluation/eval_hooks.py:147-179.",
     ["jp_confusion2", "jp_depth_eval_prepare", "jp_masked_median", "jp_depth_errors"]),
    ("Batched depth scoring and LiDAR ground truth (csrc/evalmetrics.hip, csrc/lidar.hip; core/evaluation.py::eval_depth_batch, "
     "lidar_depth_maps).  jp_depth_eval_batch: the chain of eval_depth (jp_affine -> jp_bilinear_fwd -> jp_depth_eval_prepare -> "
     "jp_masked_median x 2 -> jp_depth_errors) for B images in four launches, the same float32 operations per pixel: disp (B,1,h,w), "
     "gt (B,H,W); min_depth / max_depth are doubles because the two constants of disp_to_depth are formed in double and rounded to "
     "float once, as the Python chain does; crop rows y0..y1-1, columns x0..x1-1; fixed_scale > 0 replaces the median ratio.  sums "
     "(B,8) as jp_depth_errors defines them, med (B,4) = {n, median gt, n, median pred}: the medians are exact (radix selection, bit-"
     "equal to jp_masked_median), the sums are folded from per-workgroup partials in a fixed order, no floating-point atomics -- two "
     "runs give the same bits.  ws: jp_depth_eval_batch_ws_bytes(B, H, W) bytes, need not be initialised.  "
     "jp_lidar_depth_map: mono/datasets/kitti_utils.py::generate_depth_map for B scans in float64.  pts (sum N_b, 4) x, y, z, "
     "reflectance (not read: w = 1); offsets (B+1) in device memory, item b owns rows offsets[b] .. offsets[b+1]-1; P (B,3,4) "
     "velodyne -> image (P_rect R_rect velo2cam); flip (B) bytes or NULL: mirror the finished map left-right.  Points with x < 0 are "
     "dropped; u = rint(q0/q2) - 1, v = rint(q1/q2) - 1 (ties to even) must lie inside the image; d = q2 (vel_depth: the point's x); "
     "a pixel holds the minimum d of its points, 0 without one; negative values become 0 after the minimum.  THE QUIRK of the "
     "reference, kept because every gt_depths.npz in circulation carries it: its duplicate search gives pixel (r, W-1) and pixel "
     "(r+1, 0) one key, so when both hold points the one that owns the earliest point of the pair (file order) gets the minimum over "
     "the points of both and the other keeps the d of its own last point.  Only columns 0 and W-1 are affected (outside the Garg "
     "crop); W >= 2.  out64 / out32 (B,H,W): either may be NULL, not both; out32 is the rounded out64.  64-bit integer atomic minima "
     "on the ordered image of the double: the result does not depend on scheduling.  ws: jp_lidar_depth_ws_bytes(B, H, W) bytes; ws "
     "and the outputs need not be initialised.",
     ["jp_depth_eval_batch_ws_bytes", "jp_depth_eval_batch", "jp_lidar_depth_ws_bytes", "jp_lidar_depth_map"]),
    ("Video perception post-processing (csrc/perception.hip; apis/perception.py) — what scripts/eval_kitti_video.py does in host numpy "
     "on copied-back tensors.  jp_disp_resize_depth: disp_to_depth's scaled disparity 1/max_depth + (1/min_depth - 1/max_depth) disp, "
     "half-pixel bilinear resize to OH x OW (cv2.resize INTER_LINEAR; the sampling rule of jp_bilinear_fwd) and 1/x in one pass "
     "(:121-133); disp_out (nullable) receives the resized scaled disparity.  jp_quantiles: for every row of x (rows <= 64, n floats "
     "each) and every q[i] (HOST array, nq <= 4, in [0,1]) the order statistics k = floor(q (n-1)) and min(k+1, n-1) into out "
     "(rows, nq, 2) -- the two values numpy's `linear` quantile interpolates between (np.percentile :134; q = 0: the minimum); exact "
     "radix selection on the order-preserving key of the float (4 passes of 8 bits, integer histograms: the result does not depend "
     "on the launch order; np.sort's order: -0.0 == +0.0, +-Inf are values, NaN last); ws: jp_quantiles_ws_bytes(rows) bytes of "
     "caller scratch, need not be initialised.  jp_colorize_u8: matplotlib Normalize + 256-entry colormap (plt.imsave(cmap, vmax) "
     ":136) in fp32, idx = clamp((int)floorf((x - vmin) * (256.0f / (vmax - vmin))), 0, 255), 0 where vmax <= vmin, out = lut[idx]; "
     "vmin_vmax (rows, 2) and lut (256 x 3 bytes) in device memory, out (rows, n, 3) bytes.  jp_layout_classes_u8: np.argmax of the "
     "road and the car head (B, 2, HW; strictly-greater, ties -> 0; car_logits nullable) -> cls (B, HW) bytes 0 / 1 road / 2 car "
     "and (nullable) rgb (B, HW, 3) with the palette (0,0,0) / (255,255,255) / (0,0,255) (:157-161,195-218).",
     ["jp_disp_resize_depth", "jp_quantiles_ws_bytes", "jp_quantiles", "jp_colorize_u8", "jp_layout_classes_u8"]),
    ("Streaming perception (csrc/stream.hip; apis/stream.py PerceptionStream) -- the per-frame state of a streaming session, kept in device "
     "memory, no counterpart in the reference (scripts/eval_kitti_video.py keeps the previous frame and the global "
     "pose in host variables, :281-292).  Every launch of a frame has the same arguments as the last frame's (what a captured graph would need): both entry points read the number of frames pushed "
     "so far, n, from `count`: ONE int32 in device memory.  Ring, pose, trajectory and counter are the caller's buffers (the library "
     "keeps no state).  jp_stream_pose_pair: frame (B,3,H,W) is resized to 192 x 640 with the arithmetic of jp_bilinear_fwd "
     "(half-pixel, align_corners=False; bit-equal to it) into ring[n & 1] (ring: (2,B,3,192,640)) and into pair[:,3:6] (pair: "
     "(B,6,192,640)); pair[:,0:3] = ring[(n & 1) ^ 1], the frame of the call before, or the new frame itself when n == 0 (the demo "
     "pairs its first frame with itself) -- Baseline.predict_poses' [pf[-1], pf[0]] of frame_ids = [0, -1] in one launch, the previous "
     "frame resized only once.  amax_out: optional magnitude slot that receives max |pair| (the convention of jp_add_relu amax_out "
     "above).  count is only read.  jp_stream_traj_push: T (B,4,4) float, the cam_T_cam of frame -1 as jp_pose_fwd writes it; pose "
     "(B,16) double, the current global pose (row-major 4 x 4); traj (B,capacity,12) double.  n == 0: pose = I whatever T holds; "
     "else pose = pose @ double(T) (eval_kitti_video.py:292), every element ((a0 b0 + a1 b1) + a2 b2) + a3 b3 in float64 with each "
     "product and sum rounded once (no fma), the whole old pose read before any of it is written.  Rows 0..2 of the new pose go to "
     "traj[:, n] when n < capacity (later frames leave the trajectory alone; pose and count go on).  One thread stores count = n + 1 "
     "after every camera is done: jp_stream_pose_pair of a frame must be enqueued BEFORE its jp_stream_traj_push (one stream, or an "
     "event in between).  One workgroup, no atomics.",
     ["jp_stream_pose_pair", "jp_stream_traj_push"]),
    ("World-frame BEV map (csrc/bevmap.hip; apis/bevmap.py BevMap, PerceptionStream(bev_map=...)) -- the ego-centred class maps of a drive "
     "voted into ONE map with the drive's float64 poses; no counterpart in the reference (scripts/eval_kitti_video.py shows the current "
     "layout beside a plotted trajectory).  The map, the image and the poses are the caller's buffers (the library keeps no state).  "
     "GEOMETRY: world is the frame of camera pose T_0 = I; +X goes to increasing map columns, +Z (forward) to decreasing rows, world (0, 0) "
     "sits at cell coordinates (org_r, org_c), cells are res metres a side.  Frame cell (i, j) covers x in [(j - occ/2) res_f, "
     "(j + 1 - occ/2) res_f) and z in [(occ - 1 - i) res_f - off, (occ - i) res_f - off): row i's far edge is the forward distance of "
     + R + "net.py:230-242 (_distance_map); res_f = 40 / occ, off = 0.27 (KITTI) or 1.9 (split == 'argo').  THE BEV PLANE IS TAKEN TO "
     "BE THE CAMERA'S OWN x-z PLANE: the shift h R[.][1] from the camera's height above the ground is dropped.  "
     "jp_bev_fuse: layout (B,N,occ,occ) bytes with the classes of jp_layout_classes_u8 (0 background, 1 road, 2 car); pose: for camera b, "
     "frame n the row-major 3x4 or 4x4 camera-to-world transform at pose + (b N + n) pose_stride doubles (pose_stride 16: the session's "
     "pose; 12: trajectory rows; >= 12), of which only T[0][0], T[0][2], T[0][3], T[2][0], T[2][2], T[2][3] are read; counts (B,3,Mh,Mw) "
     "int32 [seen, road, car], read-modify-write: it accumulates over calls.  A GATHER: for map cell (r, c) and every frame, in float64 "
     "with every operation rounded once (no fma) and in exactly this order: X = ((c + 0.5) - org_c) res, Z = ((org_r - r) - 0.5) res, "
     "dX = X - T[0][3], dZ = Z - T[2][3], det = T[0][0] T[2][2] - T[0][2] T[2][0], x = (T[2][2] dX - T[0][2] dZ) / det, "
     "z = (T[0][0] dZ - T[2][0] dX) / det, u = x / res_f + occ / 2 (occ / 2 in float64: 0.5 occ), v = (z + off) / res_f; a hit iff "
     "u >= 0 && u < occ && v >= 0 && v < occ && z <= max_range, then j = floor(u), i = occ - 1 - floor(v), cls = layout[b][n][i][j]: "
     "seen += 1, road += (cls == 1), car += (cls == 2).  A frame with !(|det| >= 1e-6) contributes nothing (that covers a NaN det); every "
     "range test is false for NaN and nothing is converted to an integer before its test has passed.  The kernel does not sweep the map: per "
     "frame it visits a square window of ceil(occ res_f sqrt(2) / res) + 3 cells a side (at most 32768) whose map origin it computes ITSELF "
     "from the pose, around the footprint centre T (0, 0, occ res_f / 2 - off) (= 20 - off) -- the launch arguments of a session's push are the "
     "same for every frame; cells of the window outside the map are skipped, and so is a frame whose window misses the map or whose "
     "centre is not finite.  The window covers the footprint of every pose whose x-z block has singular values <= 1 (any rigid transform).  "
     "N == 1: one thread owns each map cell, no atomics; N > 1: the frames run in parallel with integer atomicAdd -- integer sums do not "
     "depend on the order, two runs give the same counts.  B N <= 65535.  ORDERING: enqueue a frame's jp_bev_fuse AFTER its "
     "jp_stream_traj_push on the same stream (the pose it reads is finished by that launch).  "
     "jp_bev_map_classes: counts (B,3,cells) -> cls (B,cells) bytes and (nullable) rgb (B,cells,3); counts are converted to double (exact) "
     "and the rules apply in this order: seen < min_seen -> 255; car >= car_frac seen -> 2; road + car >= road_frac seen -> 1 (a car "
     "stands on road); else 0.  Palette of jp_layout_classes_u8, and (96,96,96) for 255.  "
     "jp_bev_map_mark: traj (B,capacity,12) doubles; for each of the first n (<= capacity) rows of every camera the cell "
     "(floor(org_r - T[2][3] / res), floor(T[0][3] / res + org_c)) of rgb (B,Mh,Mw,3) is painted with color = R | G << 8 | B << 16; rows "
     "that fall outside the map or are not finite are skipped; several rows may write the same bytes to one cell.  "
     "All three refuse null pointers, non-positive sizes and res / res_f that are not greater than zero before any launch.",
     ["jp_bev_fuse", "jp_bev_map_classes", "jp_bev_map_mark"]),
    ("Depth lifted into the layout's BEV grid and depth-layout agreement (csrc/depthbev.hip; apis/depthbev.py DepthBev, "
     "PerceptionStream(depth_bev=...)) -- the inverse of the training-time warp of " + R + "net.py:193-267 (get_scale_label_static takes "
     "the BEV distance map into the image; jp_scale_label_assemble here): every depth pixel is placed in the frame-cell geometry of "
     "jp_bev_fuse above (cell (i, j) covers x in [(j - occ/2) res_f, (j + 1 - occ/2) res_f) and z in [(occ - 1 - i) res_f - off, "
     "(occ - i) res_f - off); res_f = 40 / occ, off = 0.27 (KITTI) or 1.9 (split == 'argo')).  No counterpart at inference in the "
     "reference.  Every buffer is the caller's (the library keeps no state).  "
     "jp_depth_bev_lift: depth (B,1,H,W) float metres; cam (B,8) doubles in device memory [fx, fy, cx, cy, nx, ny, nz, h]: pixel intrinsics "
     "at the resolution of depth, and the ground plane in the camera frame (height above ground of a camera-frame point P is h - n.P; "
     "(0, 1, 0, camera height) for a level camera whose y axis points down); grid (B,4,occ,occ) int32 planes [n, n_obst, hmin_mm, "
     "hmax_mm].  accumulate == 0: the call first fills grid with [0, 0, INT_MAX, INT_MIN] by a launch of its own on the same stream, the "
     "result is a pure function of the inputs; accumulate != 0: it adds to what grid holds.  Per pixel (u, v) -- integer pixel "
     "coordinates, as Backproject's meshgrid (" + R + "layers.py:41-63) -- in float64 with every operation rounded once (no fma) and in "
     "exactly this order: (1) d = (double)depth; accept iff d >= min_range && d <= max_range (false for NaN and +Inf).  "
     "(2) X = ((u - cx) / fx) d.  (3) Y = ((v - cy) / fy) d.  (4) hgt = h - ((nx X + ny Y) + nz d); accept iff hgt >= h_min && "
     "hgt <= h_max.  (5) uu = X / res_f + 0.5 occ (0.5 occ exact in float64), vv = (d + off) / res_f; accept iff 0 <= uu < occ && "
     "0 <= vv < occ.  (6) j = floor(uu), i = occ - 1 - floor(vv).  (7) q = (int)floor(hgt 1000 + 0.5).  Nothing is converted to an "
     "integer before its test has passed.  An accepted pixel updates cell (i, j) of its camera: n += 1, n_obst += (hgt > obst_h), "
     "hmin_mm = min(hmin_mm, q), hmax_mm = max(hmax_mm, q), with integer atomicAdd / atomicMin / atomicMax: order-free, two runs give "
     "the same bits.  Two forms of the kernel give the same grid: per-lane atomics, or (default; JP_DEPTH_BEV_RUNS=0 selects the "
     "other, read at every call) a wave folds each run of consecutive lanes with the same cell by a segmented scan and the run's last "
     "lane issues the atomics (profiles/depth_bev.md).  Refused before any launch: null pointers, non-positive sizes, res_f <= 0, "
     "|h_min| or |h_max| > 1e6 (heights are int32 millimetres), B H W >= 2^31, B 4 occ occ >= 2^31.  "
     "jp_depth_bev_classes: grid (B,4,cells) -> cls (B,cells) bytes, rules in this order: n < min_points -> 255 (not observed); "
     "n_obst >= obst_points -> 2 (obstacle); else 1 (ground); height (B,cells) float, nullable: (float)hmax_mm / 1000.0f (float "
     "division, rounded once), NaN where cls is 255.  "
     "jp_bev_agree: lifted, layout (B,cells) bytes -> out (B,2,3) int32, OVERWRITTEN: out[b][l-1][c] = cells with lifted == l (1 ground, "
     "2 obstacle) and layout == c (0 background, 1 road, 2 car, the classes of jp_layout_classes_u8); cells whose lifted class is 255 "
     "(or anything but 1 / 2) or whose layout value is above 2 count nowhere.  One workgroup per camera, integer sums, no atomics, no "
     "workgroup waits on another.  ORDERING in a session: the lift behind jp_disp_resize_depth, the classes behind the lift, "
     "jp_bev_agree behind both jp_depth_bev_classes and jp_layout_classes_u8, all on one stream.",
     ["jp_depth_bev_lift", "jp_depth_bev_classes", "jp_bev_agree"]),
    ("Ground plane fitted from depth (csrc/ground.hip; apis/depthbev.py DepthBev(ground=...), PerceptionStream(depth_bev=dict(ground=...))) "
     "-- the plane jp_depth_bev_lift measures heights against, estimated on the device from the depth map itself and written where the "
     "lift reads it; no counterpart in the reference (its HEIGHT_FROM_GROUND is a constant).  Every buffer is the caller's (the library "
     "keeps no state).  jp_ground_fit: depth (B,1,H,W) float metres; layout (B,occ,occ) bytes with the classes of jp_layout_classes_u8, "
     "or NULL (no road gate); prior (B,4) doubles [nx, ny, nz, h], or NULL; cam (B,8) doubles as for the lift: [0:4] = fx, fy, cx, cy "
     "are only read, [4:8] = the plane is the RESULT; part (B,parts,10) int64 scratch; mom (B,10) int64; stat (B,3) doubles.  part, mom "
     "and stat are fully overwritten: the caller zeroes nothing.  One call enqueues `rounds` pairs of launches on `stream`, a moments "
     "kernel and a solve kernel.  Round 1 gates with `prior`, or with cam[b][4:8] when prior is NULL (tracking: the last result is the "
     "next prior); later rounds gate with the plane the round before left in cam[b][4:8].  "
     "MOMENTS, per pixel (u, v) in float64 with every operation rounded once (no fma), in the lift's own order so that X, Y, d and the "
     "cell carry the same bits as there: (1) d = (double)depth; accept iff d >= min_range && d <= max_range.  (2) X = ((u - cx) / fx) d, "
     "Y = ((v - cy) / fy) d; accept iff |X| <= max_range && |Y| <= max_range.  (3) r = h - ((nx X + ny Y) + nz d) with the gating "
     "plane; accept iff r >= -band && r <= band.  (4) with a layout: uu = X / res_f + 0.5 occ, vv = (d + off) / res_f; accept iff "
     "0 <= uu < occ && 0 <= vv < occ && layout[b][occ - 1 - floor(vv)][floor(uu)] == 1 (road).  Every test is false for NaN and nothing "
     "is converted to an integer before the test that bounds it has passed.  An accepted pixel is quantised to integer millimetres, "
     "qx = (long long)floor(X 1000 + 0.5), qy from Y and qz from d likewise, and adds to TEN int64 SUMS in this order: "
     "[n, sum qx, sum qy, sum qz, sum qx qx, sum qx qz, sum qz qz, sum qx qy, sum qz qy, sum qy qy].  Integer sums are exact and do not "
     "depend on any order: the table is a pure function of the inputs whatever the grid, the wave order or `parts` (the workgroups per "
     "camera, each of which stores one row of `part`, ten zeros when it saw no pixel; no atomics, no workgroup waits on another).  "
     "SOLVE, one workgroup per camera: the rows of part are added in integers and stored to mom[b] = [n, Sx, Sy, Sz, Sxx, Sxz, Szz, Sxy, "
     "Szy, Syy]; then Y = a X + b Z + c is fitted in float64 with + - x / sqrt only, each rounded once, in exactly this order: "
     "N = (double)n; mx = Sx / N, my = Sy / N, mz = Sz / N; cxx = Sxx / N - mx mx, cxz = Sxz / N - mx mz, czz = Szz / N - mz mz, "
     "cxy = Sxy / N - mx my, czy = Szy / N - mz my, cyy = Syy / N - my my; det = cxx czz - cxz cxz; a = (cxy czz - czy cxz) / det; "
     "b = (czy cxx - cxy cxz) / det; c = my - (a mx + b mz); s = sqrt((a a + 1) + b b); plane = (-a / s, 1 / s, -b / s, (c / 1000) / s); "
     "e = cyy - (a cxy + b czy); rms = (sqrt(e > 0 ? e : 0) / s) / 1000 (metres).  STATUS CODES, the rules applied in this order: "
     "1 = too few points: n < min_points (nothing is divided).  2 = ill-conditioned: !(cxx >= sp && czz >= sp && det >= 0.01 (cxx czz)) "
     "with sp = (1000 min_spread)(1000 min_spread) -- one image row of level ground has czz = 0 and lands here.  3 = out of bounds: a "
     "component of the plane or rms is not finite, or ny < cos(max_tilt_deg pi / 180) (the host's C library cosine, passed to the "
     "kernel), or !(h >= h_lo && h <= h_hi).  0 = accepted: the plane is stored to cam[b][4:8].  On any rejection cam[b][4:8] is left as "
     "it is, except in round 1 of a call that was given `prior`, which copies prior[b] in: cam is then defined by the call alone.  "
     "stat[b] = [status, n, rms] of the LAST round, rms = NaN unless the status is 0.  Refused before any launch (-1 and a message): "
     "NULL depth, cam, part, mom or stat; non-positive B, H, W, rounds or parts, parts > 1024, non-positive occ with a layout; "
     "res_f <= 0; band not greater than zero; max_range not in (0, 1000]; (double)H W (1000 max_range)^2 >= 2^62 (the int64 sums of "
     "squares could overflow); B H W >= 2^31.  ORDERING in a session: jp_ground_fit behind jp_disp_resize_depth and "
     "jp_layout_classes_u8 (it reads both outputs), jp_depth_bev_lift behind jp_ground_fit (it reads the plane), all on one stream.",
     ["jp_ground_fit"]),
    ("BEV object instances (csrc/bevobj.hip; apis/bevobj.py BevObjects, PerceptionStream(objects=...)) -- the connected components of one "
     "class of the layout, numbered and measured on the device; no counterpart in the reference (scripts/eval_kitti_video.py paints the "
     "car cells blue and stops there).  Every buffer is the caller's (the library keeps no state).  "
     "jp_bev_objects: layout (B,occ,occ) bytes with the classes of jp_layout_classes_u8; a cell is foreground iff its byte equals "
     "cls_value (2 = car, 1 = road); conn = 4 or 8 (8: cells that touch at a corner are joined); grid: the (B,4,occ,occ) int32 planes "
     "[n, n_obst, hmin_mm, hmax_mm] of jp_depth_bev_lift, or NULL.  A component is KEPT iff it has at least min_cells cells; a smaller "
     "one (an argmax speck) is dropped before numbering: it takes no id and its cells get -1.  ID ORDER: the kept components of a camera "
     "are numbered 0, 1, 2, ... in raster order of their first cell, the smallest i occ + j.  labels (B,occ,occ) int32: the id of the "
     "kept component the cell belongs to, -1 for every other cell.  count (B) int32: the number of kept components.  OVERFLOW: count and "
     "labels are not limited by max_objects -- labels carries the full id even at or above max_objects, count[b] > max_objects tells the "
     "caller that the table is truncated.  table (B,max_objects,12) int32: row id of camera b describes object id (ids below max_objects "
     "only), rows at or beyond count[b] are zero.  THE TWELVE FIELDS of a row, in order: [cells, r_min, r_max, c_min, c_max, sum_r, "
     "sum_c, first_cell, edge_mask, pts, pts_obst, hmax_mm]: the number of cells, the bounding rows and columns (inclusive), the sums of "
     "the cells' row and column indices (the centroid is sum / cells), first_cell = i occ + j of the first cell in raster order, "
     "edge_mask bit 0 = touches row 0, bit 1 = row occ-1, bit 2 = column 0, bit 3 = column occ-1 (the object is truncated by the "
     "layout's window), pts / pts_obst = the sums of the grid's n / n_obst over the object's cells, hmax_mm = the maximum of the grid's "
     "hmax_mm over the object's cells with n > 0, INT_MIN when there is none; with grid == NULL the last three are 0, 0, INT_MIN.  "
     "The cell geometry is jp_bev_fuse's: cell (i, j) covers x in [(j - occ/2) res_f, (j + 1 - occ/2) res_f) and z in "
     "[(occ - 1 - i) res_f - off, (occ - i) res_f - off), res_f = 40 / occ.  Every output is fully overwritten: labels, count, table and "
     "ws (jp_bev_objects_ws_bytes(B, occ) bytes of caller scratch) need not be initialised.  One call enqueues five launches with "
     "fixed arguments on `stream` -- wave-local row runs, lock-free atomicMin unions of the remaining links (the root of a component is "
     "its minimum index whatever the order of arrival; every trip of the union loop lowers an index, so it ends whatever other "
     "workgroups do), flatten + sizes, one workgroup per camera for the prefix sum of the kept roots in raster order, labels + table "
     "rows -- a phase that needs a global order is a launch of its own: no workgroup waits on another.  All arithmetic is integer "
     "(atomicAdd / atomicMin / atomicMax / atomicOr): the result does not depend on any order, two runs give the same bytes.  Refused "
     "before any launch (-1 and a message): NULL layout, labels, count, table or ws; non-positive B, occ or max_objects; min_cells < 1; "
     "conn not 4 or 8; cls_value outside 0 .. 255; occ > 1024 (sum_r is an int32: 1024^2 * 1023 < 2^31); B max_objects 12 >= 2^31; "
     "B occ occ >= 2^31.  ORDERING in a session: jp_bev_objects behind jp_layout_classes_u8, and with a grid behind jp_depth_bev_lift, "
     "all on one stream.",
     ["jp_bev_objects_ws_bytes", "jp_bev_objects"]),
    ("BEV object tracks (csrc/bevtrack.hip; apis/bevtrack.py BevTracker, PerceptionStream(objects=dict(track=...))) -- the objects of "
     "jp_bev_objects associated from one frame to the next by cell overlap under the ego-motion, so that a vehicle keeps one track id "
     "while it stays in view; no counterpart in the reference.  Every buffer is the caller's (the library keeps no state): the previous "
     "frame lives in THE STATE, three buffers that every call reads and rolls forward as its last step.  "
     "jp_bev_tracks: labels (B,occ,occ) int32, count (B) int32 and table (B,max_objects,12) int32 exactly as jp_bev_objects wrote them for "
     "the current frame; pose: for camera b the current row-major 3x4 or 4x4 float64 camera-to-world transform T at pose + b pose_stride "
     "doubles (pose_stride 16: the session's pose; 12: trajectory rows).  M = max_objects, n_cur = min(count[b], M): ids >= max_objects "
     "exist in labels but are not tracked (they vote for nothing, get no row and no track id).  "
     "THE STATE: prev_labels (B,occ,occ) int32, the label map of the call before; state_i (B, 2 + 2 M) int32 = [n_prev, next_id, then for "
     "every previous object id its track_id and age]; state_d (B, 12 + 2 M) float64 = [the 12 doubles of rows 0..2 of the previous pose "
     "P, then for every previous object id its X_w and Z_w].  ZEROED STATE MEANS NO HISTORY (n_prev = 0: every object is a birth, ids "
     "from 0); n_prev is clamped to 0 .. M when read.  "
     "OVERLAP, a gather: current cells are gathered from the previous map.  overlap[b][p][c] counts, over every cell (i, j) with "
     "0 <= labels[b][i][j] = c < M and every (di, dj) in [-reach, reach]^2, the cells (i' + di, j' + dj) inside the map whose "
     "prev_labels value is p with 0 <= p < n_prev, where (i', j') is the cell of the previous camera's map that the centre of cell "
     "(i, j) falls into -- in float64 with every operation rounded once (no fma) and in exactly this order, res_f = 40 / occ: "
     "x = ((j + 0.5) - 0.5 occ) res_f, z = ((occ - 0.5) - i) res_f - off, X = (T[0][0] x + T[0][2] z) + T[0][3], "
     "Z = (T[2][0] x + T[2][2] z) + T[2][3], dX = X - P[0][3], dZ = Z - P[2][3], det = P[0][0] P[2][2] - P[0][2] P[2][0], "
     "x' = (P[2][2] dX - P[0][2] dZ) / det, z' = (P[0][0] dZ - P[2][0] dX) / det, u = x' / res_f + 0.5 occ, v = (z' + off) / res_f "
     "(jp_bev_fuse's inverse and cell rule, without its max_range test); the cell exists iff u >= 0 && u < occ && v >= 0 && v < occ, "
     "then j' = floor(u), i' = occ - 1 - floor(v); a cell whose centre falls outside the previous map votes for nothing.  Every range "
     "test is false for NaN and nothing is converted to an integer before the test that bounds it has passed.  A previous pose with "
     "!(|det| >= 1e-6) gives no votes, and so does a current pose one of whose six elements read is not finite: every object is then a "
     "birth.  overlap lives in ws (jp_bev_tracks_ws_bytes(B, occ, max_objects) = 4 B M M bytes); the call zeroes it itself.  "
     "ASSIGNMENT, greedy: repeatedly the pair (p, c), p < n_prev, c < n_cur, of largest overlap among the unused rows and columns is "
     "matched; TIE-BREAK: the smaller p, then the smaller c; it stops when the best overlap is < min_overlap.  The kernel takes the "
     "maximum of a packed 64-bit key per round and gives exactly the matches of that sequential loop.  "
     "TRACK UPDATE: a matched object inherits the track id of p and age = age of p + 1; the unmatched current objects are BIRTHS: in "
     "ascending object id each takes track = next_id++ (a counter per camera, in the state) and age = 1; the unmatched previous objects "
     "end: a track ends in the first frame it is not matched (no coasting).  "
     "OUTPUTS: tracks (B,M,4) int32, row c = [track_id, age, prev_obj (-1 for a birth), overlap (0 for a birth)], rows >= n_cur are "
     "[-1, 0, -1, 0]; kin (B,M,4) float64, row c = [X_w, Z_w, dX_w, dZ_w]: with x = ((sum_c / cells + 0.5) - 0.5 occ) res_f, "
     "z = ((occ - 0.5) - sum_r / cells) res_f - off from the object's table row (the centroid of its cell centres), "
     "X_w = (T[0][0] x + T[0][2] z) + T[0][3], Z_w = (T[2][0] x + T[2][2] z) + T[2][3], and dX_w = X_w - the stored X_w of p, "
     "dZ_w likewise, for a match, 0 for a birth; rows >= n_cur are 0; stats (B,4) int32 = [n_cur, matched, born, ended].  "
     "Every output is fully overwritten: tracks, kin, stats and ws need not be initialised.  "
     "STATE ROLL, the last step of the same call: prev_labels = labels, P = rows 0..2 of T, n_prev = n_cur, next_id += born, and per "
     "current object its track_id, age, X_w and Z_w (rows >= n_cur zero): the host swaps no pointers, every launch has the same "
     "arguments from frame to frame.  One call enqueues four launches on `stream` -- zero the matrix; the vote, one thread per current "
     "cell, its votes folded in wave-local runs and (max_objects <= 64) an LDS tile of the matrix before they reach global memory "
     "(JP_BEV_TRACKS_VOTE=0 / 1 / 2, read at every call, selects per-vote atomics / the runs / the tile: integer sums, the same matrix); "
     "the assignment, update and roll of the small state, one workgroup per camera; the copy of the label map -- a phase that needs a "
     "global order is a launch of its own: no workgroup waits on another.  The votes are integer atomicAdd and the float64 values a "
     "fixed sequence of single-rounded operations: two runs give the same bytes.  Refused before any launch (-1 and a message): a NULL "
     "pointer (all but stream are required); non-positive B, occ or max_objects; occ > 1024; max_objects > 256 (the overlap matrix and "
     "the rounds of the assignment grow with its square); reach outside 0 .. 3; min_overlap < 1; pose_stride not 12 or 16; off not "
     "finite; B occ occ >= 2^31; B max_objects max_objects >= 2^31.  jp_bev_tracks_ws_bytes returns 0 for a non-positive argument.  "
     "ORDERING in a session: jp_bev_tracks behind jp_bev_objects (it reads labels, count and table) and behind jp_stream_traj_push (the "
     "pose it reads is finished by that launch), all on one stream.",
     ["jp_bev_tracks_ws_bytes", "jp_bev_tracks"]),
    ("Filtered BEV tracks (csrc/bevfilter.hip; apis/bevfilter.py BevTrackFilter, PerceptionStream(objects=dict(track=dict(filter=...)))) "
     "-- a stage behind jp_bev_tracks that coasts its tracks through missed frames, repairs its id switches and filters their motion: "
     "a persistent id (fid), a life cycle tentative -> confirmed -> coasting -> ended, and per world axis a constant-velocity Kalman "
     "filter; no counterpart in the reference.  Every buffer is the caller's (the library keeps no state): THE STATE is also the output, "
     "every call reads it and rolls it forward.  "
     "jp_bev_track_filter reads what jp_bev_tracks wrote for the current frame and never a label map: tracks (B,M,4) int32, kin (B,M,4) "
     "float64, stats (B,4) int32; M = max_objects, S = max_tracks.  "
     "THE STATE, three row layouts: slots_i (B,S,8) int32, row s = [fid, status, src_track, age, hits, misses, obj, 0], status 0 free, "
     "1 tentative, 2 confirmed, 3 coasting, src_track the jp_bev_tracks id the slot follows, obj the current object id or -1 while "
     "coasting; slots_d (B,S,10) float64, row s = [X, Z, vX, vZ, aX, bX, cX, aZ, bZ, cZ], metres and metres per frame, the two axes "
     "decoupled, each with the symmetric covariance [[a, b], [b, c]] of [position, velocity]; head (B,2) int32 = [next_fid, calls].  "
     "ZEROED STATE MEANS NO HISTORY (every slot free, fids from 0).  A slot is LIVE iff its status is 1, 2 or 3; the row of a slot that "
     "is not live when the call ends is written as zeros whatever it held.  "
     "OUTPUTS, fully overwritten (they need not be initialised): obj_slot (B,M) int32, the slot of current object c or -1; fstats (B,8) "
     "int32 = [live, confirmed, coasting, continued, reacquired, born, ended, dropped].  "
     "With r = meas_sigma meas_sigma, q = accel_sigma accel_sigma, c0 = vel_sigma0 vel_sigma0 and gate gate -- each squared once inside "
     "the call, one rounded multiply -- a call does, per camera, exactly this sequential definition.  "
     "0. OBJECTS: n = min(max(stats[b][0], 0), M); object c < n has t_c = tracks[b][c][0] and the measurement z_c = (kin[b][c][0], "
     "kin[b][c][1]); it is VALID iff both are finite, an invalid object is ignored everywhere.  No value read from device memory is used "
     "as an index before it is range-checked; track ids are only compared.  "
     "1. PREDICT every live slot, per axis: p' = p + v, v' = v, a' = ((a + (b + b)) + c) + q/4, b' = (b + c) + q/2, c' = c + q.  "
     "2. CONTINUE: valid object c is bound to slot s iff s is live with misses == 0 and src_track == t_c; the ids of jp_bev_tracks are "
     "unique within a frame and never reused, so there is at most one such slot (for any other state: a slot picks the smallest such c, "
     "and c is bound to the smallest slot that picked it).  "
     "3. RE-ACQUIRE: the candidate slots are the live slots not bound in step 2 (the coasting ones, and those whose tracker track ended "
     "in this very frame: the id-switch repair), the candidate objects the valid unbound ones; dx = z_c.X - X', dz = z_c.Z - Z' from the "
     "PREDICTED position, d2 = dx dx + dz dz (two rounded products, one rounded sum); a pair qualifies iff d2 <= gate gate (false for "
     "NaN); greedy: repeatedly the qualifying pair of smallest d2 among the unused slots and objects is matched, TIE-BREAK: the smaller "
     "slot index, then the smaller object id, until no pair qualifies; a match rebinds src_track = t_c.  "
     "4. BIRTHS: the remaining valid unbound objects, in ascending object id, take the slots that were free at entry of the call, in "
     "ascending slot index (a slot freed in step 6 of a call is taken in the next call at the earliest); each takes fid = next_fid++ in "
     "that order; objects that find no slot are counted in dropped and take no fid.  Initial state: position = measurement, velocity 0, "
     "covariance [[r, 0], [0, c0]] per axis, src_track = t_c, age = hits = 1, misses = 0.  "
     "5. UPDATE the bound and the re-acquired slots from the predicted state, per axis with the measurement z: y = z - p', S = a' + r, "
     "K1 = a' / S, K2 = b' / S, p = p' + K1 y, v = v' + K2 y, a = a' - K1 a', b = b' - K1 b', c = c' - K2 b'; age++, hits++, "
     "misses = 0, obj = c.  "
     "6. MISS, the live slots still unbound: a tentative slot, or one with misses + 1 > max_coast, is freed (its whole row zeroed, "
     "counted in ended); any other keeps the predicted state with misses++, age++, status = 3, obj = -1.  "
     "7. STATUS of every slot that has a measurement (steps 4 and 5): 2 if hits >= min_hits, else 1.  "
     "Then fstats: live, confirmed and coasting count the slots by status as the call leaves them, continued / reacquired / born / ended / "
     "dropped the decisions of steps 2, 3, 4, 6 and 4; head = [next_fid, calls + 1].  "
     "ARITHMETIC: float64, every operation rounded once (no fma), in the order written; the result is a pure function of the arguments "
     "and the state: two runs give the same bytes.  One call is ONE launch with fixed arguments on `stream`, grid (B): one workgroup per "
     "camera, one thread per slot and per object, no atomics, no workspace; no workgroup waits on another.  The S x M distances are never "
     "stored: a slot keeps its nearest free object and rescans when another slot takes it, a round is one minimum over the bit pattern "
     "of the non-negative d2.  Refused before any launch (-1 and a message): a NULL pointer (all but stream are required); non-positive "
     "B, max_objects or max_tracks; max_objects > 256; max_tracks > 256; max_coast < 0; min_hits < 1; gate, vel_sigma0 or accel_sigma "
     "not finite or negative; meas_sigma not finite or not greater than zero; B max_tracks 10 >= 2^31; B max_objects 4 >= 2^31.  "
     "ORDERING in a session: jp_bev_track_filter behind jp_bev_tracks (it reads tracks, kin and stats), on one stream.  RESET BOTH: "
     "resetting the tracker without resetting the filter lets stale src_track values match new tracks (the tracker numbers its tracks "
     "from 0 again).",
     ["jp_bev_track_filter"]),
    ("KITTI odometry evaluation (csrc/odometry.hip; core/evaluation.py::eval_odometry, apis/inference.py) — the pose chaining of "
     "scripts/draw_odometry.py:62-76 and the numpy toolkit behind the paper's t_err / r_err (mono/tools/kitti_evaluation_toolkit.py:"
     "109-201, mono/tools/geometry.py:20-67, scripts/plot_kitti.py:15-97,223-243).  All arithmetic is double, no atomics: every sum "
     "and product is folded in an order that depends on n alone (two runs are bit-identical); scans are three launches (block-local, "
     "one workgroup over the block aggregates, apply), no workgroup waits on another.  A pose is the 12 doubles of rows 0..2 of a 4x4, "
     "the KITTI text layout.  jp_pose_chain_f64: T (n,4,4) float frame-to-frame transforms as jp_pose_fwd writes them (row 3 is not "
     "read: 0 0 0 1) -> poses (n+1,12), G_0 = I, G_k = G_{k-1} M_k with M_k = T_k^-1 (invert != 0; the GENERAL affine inverse, "
     "adjugate / determinant, not the transpose) or T_k; ws: jp_pose_chain_ws_bytes(n) bytes.  jp_odom_segment_errors: gt / pred (n,12); "
     "lengths: HOST array of nlen <= 16 positive lengths in metres; dist (n) = trajectoryDistances of gt; with S = ceil(n / step) start "
     "frames s step: last_frame (S nlen) = first i >= first with dist[i] > dist[first] + len (bisection; -1: the sequence is too short), "
     "table (S nlen, 5) rows [first_frame, r_err / len, t_err / len, len, speed] of calcSequenceErrors, untouched where last_frame is -1; "
     "r_err = acos(clamp((trace - 1) / 2, -1, 1)), speed = len / (0.1 (last - first + 1)); ws: jp_odom_segments_ws_bytes(n, step, nlen) "
     "bytes.  jp_traj_moments: positions (columns 3, 7, 11) of x / y (n,12) -> out (19): mean_x, mean_y, sigma_x^2 = 1/n sum |x - "
     "mean_x|^2, cov = 1/n sum (y - mean_y)(x - mean_x)^T (row-major), sum x.y, sum x.x, sum |x - y|^2 -- two passes, means first "
     "(Umeyama eq. 34-38; plot_kitti's scale; the ATE); ws: jp_traj_moments_ws_bytes(n) bytes.  jp_poses_transform_f64: "
     "out_k = A [R_k | scale t_k], A: HOST array of 12 doubles; A = I is traj.scale(scale) exactly; out may be poses.  Scratch need "
     "not be initialised.",
     ["jp_pose_chain_ws_bytes", "jp_pose_chain_f64", "jp_odom_segments_ws_bytes", "jp_odom_segment_errors", "jp_traj_moments_ws_bytes",
      "jp_traj_moments", "jp_poses_transform_f64"]),
    ("Device-side input pipeline — MonoDataset.preprocess mono/datasets/mono_dataset.py:126-171 (PIL ANTIALIAS resize, bit-exact "
     "Pillow fixed-point resampler; ToTensor; ColorJitter in torchvision tensor arithmetic) and process_topview :417-431, applied "
     "to raw uint8 frames after one pinned async upload.  *_flip: MonoDataset.__getitem__'s do_flip (mono_dataset.py:203; every getter's "
     "transpose(pil.FLIP_LEFT_RIGHT) of the raw image / BEV label BEFORE any resize) per item of a batch: flip = N bytes in device memory, "
     "non-zero = mirror that item left-right before the operation, NULL = no item; with NULL or all-zero flags the output is bit-identical "
     "to the plain entry point's.  jp_resample_h_u8_flip: jp_resample_h_u8 over N items of H rows, a flagged item's tap k of output "
     "column ox reads source column W-1-(xmin+k) (= resizing the mirrored image, bit for bit).  jp_u8_to_tensor_flip: no horizontal "
     "resize -- writes the float CHW / 255 tensor (dst_f) and / or the mirrored uint8 HWC image (dst_u8); either may be NULL, not both; "
     "dst_u8 != src.  jp_topview_u8_flip: the NEAREST pick of jp_topview_u8 on the mirrored label (column w-1-sx).  "
     "jp_color_jitter_batched: ColorJitter on N images (N,3,HW) in place, two launches whatever N is; params (N, 9) int32 in device "
     "memory, one record per image: n_ops (0..4; 0 = the image is not written), order[4] (op ids 0 brightness / 1 contrast / "
     "2 saturation / 3 hue in the order they are applied, contrast at most once), factor[4] (bit patterns of the floats, factor[j] "
     "belongs to order[j]).  Contrast blends with the gray mean of the image as it stands after the ops before it: the first launch "
     "recomputes those per pixel and leaves per-workgroup partial sums in ws (jp_color_jitter_batched_ws_doubles(N, HW) doubles of "
     "caller scratch, need not be initialised), the second folds them in a fixed order -- no atomics, two runs give the same bits "
     "(jp_color_jitter_op folds its gray sum with atomic adds).",
     ["jp_resample_h_u8", "jp_resample_v_u8", "jp_u8_to_tensor", "jp_color_jitter_op", "jp_topview_u8", "jp_resample_h_u8_flip",
      "jp_u8_to_tensor_flip", "jp_topview_u8_flip", "jp_color_jitter_batched_ws_doubles", "jp_color_jitter_batched"]),
    ("Library plumbing.  jp_profile_*: opt-in per-kernel HIP-event timing on the streams the kernels are launched on (bench.py's "
     "roofline leg; never active in the train step).  Recorded are the implicit-GEMM launches (tag = the launch helper's "
     "instantiation, flops = executed FLOPs of the GEMM) and two element-wise kernels of the eval-mode forward, jp_bn_eval_fwd "
     "and jp_add_relu (tag = the entry point's name, flops = 0: they run no GEMM; tools/frozen_bench.py compares them).",
     ["jp_abi_version", "jp_last_error_string", "jp_set_last_error", "jp_profile_begin", "jp_profile_count", "jp_profile_end",
      "jp_profile_get"]),
]


def collect():
    protos = {}
    for f in sorted(glob.glob(os.path.join(ROOT, "jperceiver_amd/csrc/*.hip")) + [os.path.join(ROOT, "jperceiver_amd/csrc/capi.cpp")]):
        src = open(f).read()
        for m in re.finditer(r'extern "C" ((?:const )?\w+\*?) (jp_\w+)\(([^)]*)\)\s*\{', src):
            ret, name, args = m.group(1), m.group(2), " ".join(m.group(3).split())
            protos[name] = f"{ret} {name}({args});"
    return protos


def main():
    protos = collect()
    out = ["/* jperceiver_hip.h — C ABI of libjperceiver_hip.so (MI355X / gfx950 only).",
           " *",
           " * GENERATED by tools/gen_header.py from jperceiver_amd/csrc — do not edit by hand.",
           " *",
           " * Drop-in boundary for the JPerceiver `Baseline` training step (SURVEY.md §8b): the reference has no",
           " * native layer of its own (pure PyTorch), so these entry points are what a ctypes binding inside",
           " * mono/model/mono_baseline/* would call in place of the ATen/cuDNN ops cited per group.",
           " *",
           " * Conventions: fp32 NCHW contiguous tensors; raw device pointers; explicit int dims; every call is",
           " * enqueued on `stream` (a hipStream_t passed as void*), never synchronises and never allocates —",
           " * the caller owns all buffers including scratch; no entry point keeps state for a later call (the only",
           " * thread-local data are the error string and the opt-in pack recorder / profiler).  Return 0 on success, <0 for a bad argument, >0 =",
           " * hipError_t; jp_last_error_string() describes the last failure on the calling thread.",
           " * `gout` arguments are device pointers to the upstream scalar gradient (NULL = 1.0).",
           " */",
           "#ifndef JPERCEIVER_HIP_H", "#define JPERCEIVER_HIP_H", "#include <stdint.h>", "",
           "#ifdef __cplusplus", 'extern "C" {', "#endif", ""]
    seen = set()
    for doc, names in GROUPS:
        out.append("/* " + "\n * ".join(_wrap(doc)) + " */")
        for n in names:
            out.append(protos[n])
            seen.add(n)
        out.append("")
    missing = set(protos) - seen
    assert not missing, f"ungrouped entry points: {missing}"
    out += ["#ifdef __cplusplus", "}", "#endif", "#endif /* JPERCEIVER_HIP_H */", ""]
    with open(os.path.join(ROOT, "include", "jperceiver_hip.h"), "w") as f:
        f.write("\n".join(out))
    print("wrote", len(protos), "prototypes")


def _wrap(s, width=108):
    words, lines, cur = s.split(), [], ""
    for w in words:
        if len(cur) + len(w) + 1 > width:
            lines.append(cur)
            cur = w
        else:
            cur = (cur + " " + w).strip()
    lines.append(cur)
    return lines


if __name__ == "__main__":
    main()
