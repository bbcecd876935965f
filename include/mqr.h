/*
 * mqr.h -- C ABI of libmqr_hip.so, the MI355X (gfx950) TSDF fusion path.
 *
 * Drop-in boundary for the reference's Open3D VoxelBlockGrid usage and its numpy confidence
 * estimator (lszmer/metaquest-3d-reconstruction).  Each entry point names the reference
 * interface it replaces.  Conventions:
 *   - every function returns 0 on success, non-zero on error; mqr_last_error() returns a
 *     thread-local message (the Python layer raises RuntimeError with it, as Open3D does);
 *   - plain pointers and sizes only; `loc` arguments say where a buffer lives:
 *     MQR_HOST (caller-owned host memory, read/written during the call only) or
 *     MQR_DEVICE (device pointer on the volume's device, e.g. from mqr_device_alloc);
 *   - stream ordering of MQR_DEVICE buffers: the library runs on its own non-blocking HIP streams.
 *     Every call that reads or writes caller device buffers first makes those streams wait for all
 *     work enqueued so far on the calling thread's CALLER STREAM (mqr_set_stream; default: the null
 *     stream), so a kernel or copy the caller enqueued there that writes an input -- or still reads a
 *     buffer the call overwrites -- is complete before the library touches it.  No host wait is
 *     involved (an event and a stream wait).  Every call but one has finished with its buffers when
 *     it returns: outputs are complete and visible to any stream afterwards.  The exception is
 *     mqr_integrate_frames on MQR_DEVICE frames, which returns once its last integrate is queued:
 *     the caller stream is then made to wait (device-side) for that integrate, so whatever the
 *     caller enqueues there next -- overwriting or freeing the frames included -- runs after the
 *     library's reads; every later call on the volume orders itself behind it (a host-side reader
 *     of the frames synchronizes the caller stream first, as it would for a kernel of its own).
 *     mqr_integrate_frames also takes MQR_DEVICE_RESIDENT frames: device frames the caller keeps
 *     allocated and unchanged until the device (or the volume, by any call that drains it) has been
 *     synchronized -- e.g. a capture uploaded once and integrated pass after pass.  Reads are ordered
 *     after the caller stream as for MQR_DEVICE, but the caller stream is not made to wait for the
 *     call's integrates, so the next call's first touch -- itself behind the caller stream -- can run
 *     beside this call's last integrate instead of after it;
 *   - matrices are row-major: K = 3x3 intrinsic (Open3D convention, cx already flipped),
 *     T_wc = 4x4 world->camera extrinsic, both float64 as the reference passes them
 *     (o3d_utils.py:203-210);
 *   - a volume handle is not re-entrant; several handles per process/device are fine.
 */
#ifndef MQR_H
#define MQR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MQR_HOST 0
#define MQR_DEVICE 1
#define MQR_DEVICE_RESIDENT 2 /* mqr_integrate_frames only: see "stream ordering" above */

typedef struct mqr_vbg mqr_vbg;    /* voxel-block-hashed TSDF volume resident in HBM */
typedef struct mqr_geom mqr_geom;  /* extracted point cloud or triangle mesh (device-resident) */
typedef struct mqr_scene mqr_scene;  /* triangle-mesh ray-casting scene (device BVH) */
typedef struct mqr_comm mqr_comm;    /* RCCL communicator of one rank (one process per GPU) */

int mqr_version(void);
/* Build tags: which 0 = a hash of the integrate sources (vbg.hip, vbg_kernels.hpp, mqr_common.hpp),
 * 1 = of the confidence sources, as compiled into this library; counter records under profiles/ carry
 * the tag of the build they measured (bench.py quotes only matching ones).  mqr_vbg_last_kernel: the
 * integrate variant (mqr_vbg_set_variant numbering) the volume's last launch actually used.
 * mqr_vbg_flips: how many mqr_vbg_reset calls swapped in the volume's second table / pool set instead of
 * waiting for an integrate still in flight (see mqr_vbg_reset). */
int mqr_build_tag(int which, char* buf, int cap);
int mqr_vbg_last_kernel(mqr_vbg* v, int* variant);
/* The name of the main kernel the volume's last integrate launch ran (e.g. "k_integrate_wt<7, 1>"). */
int mqr_vbg_last_kernel_name(mqr_vbg* v, char* buf, int cap);
int mqr_vbg_flips(mqr_vbg* v, int64_t* n);
const char* mqr_last_error(void);
int mqr_device_count(int* n);
/* The calling thread's caller stream (a hipStream_t; NULL = the null stream, the default): see
 * "stream ordering" above.  A PyTorch caller passes torch.cuda.current_stream().cuda_stream (the
 * Python layer does this by itself).  A caller stream of another device than the call's is drained on
 * the host instead (hipStreamSynchronize; no cross-device stream wait); an invalid one is status 2.
 * mqr_get_stream reads the current setting. */
int mqr_set_stream(void* stream);
int mqr_get_stream(void** stream);

/* Device memory helpers (so callers can keep inputs resident in HBM without any framework).
 * mqr_device_free waits for the device first (work in flight may still read the buffer). */
int mqr_device_alloc(int device, int64_t bytes, void** ptr);
int mqr_device_free(int device, void* ptr);
int mqr_memcpy(void* dst, int dst_loc, const void* src, int src_loc, int64_t bytes, int device);
int mqr_device_synchronize(int device);
/* hipMemGetInfo of `device`: free and total HBM bytes (the Python layer keeps a released volume for
 * reuse only while enough stays free). */
int mqr_device_mem_info(int device, int64_t* free_bytes, int64_t* total_bytes);

/* o3d.t.geometry.VoxelBlockGrid(attr_names=('tsdf','weight'), attr_dtypes=(f32,f32), attr_channels=(1,1),
 *                               voxel_size, block_resolution, block_count, device)
 * -- reference call site scripts/processing/reconstruction/utils/o3d_utils.py:170-179.
 * block_count is the initial capacity; the volume grows automatically like Open3D's hash map. */
int mqr_vbg_create(float voxel_size, int block_resolution, int64_t block_count, int device, mqr_vbg** out);
/* The same volume with Open3D's attr_names=('tsdf','weight','color') layout: one more attribute per voxel,
 * three float32 channels in 0..255, every channel 0 whenever a block is allocated or the volume is reset
 * (DESIGN.md 2.11).  block_resolution must be 8 or 16 (else status 2).  Costs 20 bytes per voxel instead of 8.
 * A coloured volume's mqr_vbg_reset never swaps sets: it queues behind an unfinished integrate.  The multi-GPU
 * merge (mqr_vbg_pack_weighted / unpack_weighted, mqr_reduce_rccl, mqr_merge_local, mqr_xchg_*) and
 * mqr_extract_mesh_owned refuse a coloured volume with status 2. */
int mqr_vbg_create_color(float voxel_size, int block_resolution, int64_t block_count, int device, mqr_vbg** out);
int mqr_vbg_has_color(mqr_vbg* v, int* has_color);
int mqr_vbg_destroy(mqr_vbg* v);
/* Empty the volume in place (keeps its allocations): the state of a freshly created grid.  Ordered on the
 * device: when an integrate of an asynchronously returning mqr_integrate_frames is still in flight, the
 * volume swaps in a second hash table / block pool set (allocated once, at the current capacities, while the
 * volume's pool is within 2 GiB and a quarter of the device's HBM stays free) and clears that one, so the
 * next call's first touch overlaps the unfinished integrate; otherwise the clear queues behind it. */
int mqr_vbg_reset(mqr_vbg* v);
int mqr_vbg_size(mqr_vbg* v, int64_t* n_blocks);
int mqr_vbg_capacity(mqr_vbg* v, int64_t* block_capacity);
int mqr_vbg_params(mqr_vbg* v, float* voxel_size, int* block_resolution, int* device);

/* vbg.compute_unique_block_coordinates(depth, intrinsic, extrinsic, depth_scale, depth_max,
 *                                      trunc_voxel_multiplier)  -- o3d_utils.py:212-219.
 * keys_out (host) must hold 4*(H/4)*(W/4) int32 triplets.  Returns 3 ("no block is touched")
 * when nothing is touched, like upstream.  The main volume is not modified. */
int mqr_touch(mqr_vbg* v, const float* depth, int depth_loc, int H, int W, const double* K, const double* T_wc,
              float depth_scale, float depth_max, float trunc_mult, int32_t* keys_out, int64_t* n_out);

/* vbg.integrate(block_coords, depth, intrinsic, extrinsic, depth_scale, depth_max,
 *               trunc_voxel_multiplier)  -- o3d_utils.py:221-229.  keys: n int32 triplets (host). */
int mqr_integrate(mqr_vbg* v, const int32_t* keys, int64_t n, const float* depth, int depth_loc, int H, int W,
                  const double* K, const double* T_wc, float depth_scale, float depth_max, float trunc_mult);

/* The whole per-frame loop of o3d_utils.integrate (:188-236): touch + integrate for B frames in
 * order, batched on device (results identical to B sequential touch+integrate calls).
 * depths: B*H*W float32 metric depth (0 = invalid), K: B*9, T_wc: B*16 (host float64).
 * frame_ok (host, may be NULL): frames with frame_ok[i]==0 are skipped (missing/invalid loads).
 * Returns 3 if a valid frame touches no block (upstream raises).  Every batch's touch counters are
 * read on the host before its integrate is launched, so errors are reported by this call; with
 * MQR_DEVICE / MQR_DEVICE_RESIDENT frames the call returns with the last integrate still running (see
 * "stream ordering" above), with MQR_HOST frames after it has finished. */
int mqr_integrate_frames(mqr_vbg* v, const float* depths, int depth_loc, int B, int H, int W, const double* K,
                         const double* T_wc, const uint8_t* frame_ok, float depth_scale, float depth_max,
                         float trunc_mult);

/* Open3D's colour integrate: vbg.integrate(block_coords, depth, color, depth_intrinsic, color_intrinsic,
 * extrinsic, ...).  The (tsdf, weight) update is mqr_integrate's / mqr_integrate_frames', bit for bit; a voxel
 * that accepts a frame and projects into the colour image (its own intrinsic K_color, the depth's extrinsic)
 * also averages that pixel into its colour with the weight before the update.
 * colors: uint8 [B][Hc][Wc][3] (one frame for mqr_integrate_color), color_loc MQR_HOST or MQR_DEVICE; K_color B*9.
 * Host colour frames are staged per batch as host depth frames are.  With depth and colour both MQR_DEVICE the
 * call orders itself behind the caller stream and returns with the last integrate queued, the caller stream
 * made to wait for it, as mqr_integrate_frames does; otherwise it returns when the work has finished
 * (MQR_DEVICE_RESIDENT is not accepted).  A volume without colour, a null pointer, Hc or Wc <= 0, a non-finite
 * K_color or one with a zero focal length: status 2, nothing launched.  The depth-only calls stay legal on a
 * coloured volume and leave its colours alone. */
int mqr_integrate_color(mqr_vbg* v, const int32_t* keys, int64_t n, const float* depth, int depth_loc, int H, int W,
                        const uint8_t* color, int color_loc, int Hc, int Wc, const double* K_depth,
                        const double* K_color, const double* T_wc, float depth_scale, float depth_max,
                        float trunc_mult);
int mqr_integrate_frames_color(mqr_vbg* v, const float* depths, int depth_loc, int B, int H, int W,
                               const uint8_t* colors, int color_loc, int Hc, int Wc, const double* K_depth,
                               const double* K_color, const double* T_wc, const uint8_t* frame_ok, float depth_scale,
                               float depth_max, float trunc_mult);

/* Volume contents (VoxelBlockGrid.save / load payload, and the multi-GPU merge).  Blocks are in
 * buffer order: keys n*3 int32, tsdf / weight n*R^3 float32 ([z][y][x] within a block). */
int mqr_vbg_export(mqr_vbg* v, int32_t* keys, float* tsdf, float* weight, int loc);
int mqr_vbg_import(mqr_vbg* v, const int32_t* keys, const float* tsdf, const float* weight, int64_t n, int loc);
/* Colours of a coloured volume: n*R^3*3 float32, [block][voxel][channel] with the blocks in mqr_vbg_export's
 * order, whatever the pool's own layout.  import_color writes the colours of the blocks `keys` names (blocks
 * the volume does not hold are skipped); mqr_vbg_import itself leaves the colours of the blocks it allocates
 * at zero.  A volume without colour: status 2. */
int mqr_vbg_export_color(mqr_vbg* v, float* colors, int loc);
int mqr_vbg_import_color(mqr_vbg* v, const int32_t* keys, const float* colors, int64_t n, int loc);

/* Multi-GPU merge: pack the volume against a shared, sorted union key table into
 * [U][R^3][2] = (weight*tsdf, weight) float32 (zeros where a block is absent), and the inverse
 * after a sum-reduce: tsdf = sum(w*tsdf)/sum(w), weight = sum(w).  Device pointers. */
int mqr_vbg_pack_weighted(mqr_vbg* v, const int32_t* union_keys, int64_t U, float* packed);
int mqr_vbg_unpack_weighted(mqr_vbg* v, const int32_t* union_keys, int64_t U, const float* packed);

/* The single exchange step of frame-sharded fusion (SURVEY §8(b) mqr_reduce_rccl, §8(e)); the
 * reference has no distributed path -- this replaces running its integrate() loop
 * (o3d_utils.py:153-238) over all frames in one process.  One process per GPU: rank 0 makes an id
 * (mqr_comm_unique_id), the caller distributes it (e.g. a gloo / TCP store), every rank calls
 * mqr_comm_init.  RCCL (librccl.so.1) is resolved at run time.
 * mqr_reduce_rccl merges every rank's `local` volume into `out` (emptied first):
 *   MQR_MERGE_ROOT     `out` on `root` holds the whole merged volume (others: empty);
 *   MQR_MERGE_SHARDED  `out` holds this rank's owned slice of the sorted block union first
 *                      (*n_owned blocks), then the one-block halo; extract it with
 *                      mqr_extract_mesh_owned(out, thr, *n_owned): shard meshes concatenate to the
 *                      single-volume mesh (triangle counts add exactly).
 * Voxels seen by one rank keep its (tsdf, weight) bit for bit; others merge in rank order:
 * tsdf = (w_a tsdf_a + w_b tsdf_b) / (w_a + w_b), weight = w_a + w_b.  `out` must not be `local`.
 * The plan (sorted block union, owner slices, halo sets, send / receive lists) is computed on the
 * device; the host reads only block counts and list lengths.
 * mqr_comm_timing: the last merge's phases in ms -- [0] count + key all-gathers and the plan,
 * [1] output volume + gather of the outgoing blocks, [2] the RCCL exchange, [3] the merge kernels.
 * mqr_merge_local: the same exchange for n volumes of one process on one device, with device copies
 * as the transport: every rank builds its own plan, packs its own send segments and merges its
 * receive segments in rank order exactly as mqr_reduce_rccl does on that rank; before a byte moves,
 * each sender's segment for d is checked against d's receive segment from it (length, and the
 * source buffers both sides list, entry for entry; mismatch = status 4).  Tests and timing.
 * mqr_merge_local_timing: the last mqr_merge_local's wall time per rank in ms (its plan, output
 * volume, send-segment gather and merge kernels: one rank's share of a merge, without the transfer).
 *
 * mqr_xchg_*: the same exchange with the transport left to the caller (one process per rank; the
 * tests carry the segments over gloo through host buffers).  gathered_keys: world*mx packed block
 * keys (rank r's keys in buffer order at r*mx, padded with 0xFFFF...FF; packing as the int32 keys
 * of mqr_vbg_export: ((x+2^20)<<42)|((y+2^20)<<21)|(z+2^20)).  create = plan + output volume
 * (emptied) + send segments (+ the self segment in place); counts[world] = blocks per send segment
 * (to each peer) and per receive segment (from each peer), floats_per_block = 2*R^3 ((tsdf,
 * weight) interleaved); send_segment copies the segment for `peer` out, recv_segment copies the
 * segment from `peer` in (peer != rank); finish merges in rank order.  `out` must outlive the
 * handle. */
#define MQR_MERGE_ROOT 0
#define MQR_MERGE_SHARDED 1
int mqr_comm_unique_id(uint8_t* id_out /* 128 bytes */);
int mqr_comm_init(int device, int rank, int world, const uint8_t* id /* 128 bytes */, mqr_comm** out);
int mqr_comm_destroy(mqr_comm* comm);
int mqr_reduce_rccl(mqr_vbg* local, mqr_comm* comm, int mode, int root, mqr_vbg* out, int64_t* n_owned);
int mqr_merge_local(mqr_vbg** locals, int n, int mode, int root, mqr_vbg** outs, int64_t* n_owned);
int mqr_comm_timing(mqr_comm* comm, float* ms4);
/* Segment sizes of the last mqr_reduce_rccl on `comm`: blocks sent to / received from each rank
 * (world entries each; the own rank's entry is the local self segment, not carried by RCCL) and the
 * 4-byte words per block (2 R^3, or 1.5 R^3 with uint16 weights).  Zeros before the first merge. */
int mqr_comm_counts(mqr_comm* comm, int64_t* send_blocks, int64_t* recv_blocks, int64_t* floats_per_block);
int mqr_merge_local_timing(float* ms, int n);
/* Merge A/B and test hooks (process-wide).  Bit 0: how every transport merges the received segments --
 * 0 (default) one fused pass per output block folding its entries in rank order in registers, 1 the
 * round-5 form, one pass over the output per source rank.  Bit 1: mqr_merge_local sends float32 weights
 * even where uint16 would hold them.  Segment format: a block travels as its R^3 (tsdf, weight) float32
 * pairs, or -- when every rank's weights are integers <= 65535, which the library knows from each volume's
 * frame count (volumes filled by import or unpack count as unknown) -- as R^3 float32 tsdf then R^3
 * uint16 weights (6 B instead of 8 B per voxel); mqr_comm_counts / mqr_xchg_counts report the 4-byte
 * words per block of the format used (2 R^3 or 1.5 R^3; the caller-carried transport always uses float32
 * pairs).  Every combination gives the same bits. */
int mqr_merge_set_per_source(int on);
typedef struct mqr_xchg mqr_xchg;
int mqr_xchg_create(mqr_vbg* local, int world, int rank, int mode, int root, const uint64_t* gathered_keys,
                    int64_t mx, int keys_loc, mqr_vbg* out, mqr_xchg** h);
int mqr_xchg_counts(mqr_xchg* h, int64_t* send_blocks, int64_t* recv_blocks, int64_t* n_owned,
                    int64_t* floats_per_block);
int mqr_xchg_send_segment(mqr_xchg* h, int peer, float* dst, int loc);
int mqr_xchg_recv_segment(mqr_xchg* h, int peer, const float* src, int loc);
int mqr_xchg_finish(mqr_xchg* h, int64_t* n_owned);
int mqr_xchg_destroy(mqr_xchg* h);

/* vbg.extract_point_cloud(weight_threshold=3.0)   -- reconstruct_scene.py:90, refine_fragment_poses.py:39
 * vbg.extract_triangle_mesh(weight_threshold)       -- reconstruct_scene.py:105-108, 186-189 */
int mqr_extract_points(mqr_vbg* v, float weight_threshold, mqr_geom** out);
int mqr_extract_mesh(mqr_vbg* v, float weight_threshold, mqr_geom** out);
/* Triangles only of cubes whose origin voxel lies in blocks [0, n_owned) (a shard from
 * mqr_reduce_rccl MQR_MERGE_SHARDED); vertices of every block (unreferenced ones may remain). */
int mqr_extract_mesh_owned(mqr_vbg* v, float weight_threshold, int64_t n_owned, mqr_geom** out);
int mqr_geom_counts(mqr_geom* g, int64_t* n_vertices, int64_t* n_triangles);
/* Copy to caller buffers (positions / normals n*3 float32, triangles n*3 int32); NULL skips. */
int mqr_geom_copy(mqr_geom* g, float* positions, float* normals, int32_t* triangles, int loc);
int mqr_geom_free(mqr_geom* g);
/* The geometry's arrays in place (device pointers on its device, null when empty; valid until
 * mqr_geom_free, and only after the call that produced it returned): positions / normals float32
 * [nv][3], triangles int32 [nt][3].  Lets a caller keep the result in HBM, as Open3D's tensor geometry
 * on a CUDA device stays there, and hand it to MQR_DEVICE inputs (mqr_scene_add_triangles,
 * mqr_mesh_filter_components, mqr_color_map) without a host round trip. */
int mqr_geom_device_ptrs(mqr_geom* g, void** positions, void** normals, void** triangles);
/* Vertex colours of a result (float32 [nv][3], 0..1).  mqr_extract_points / mqr_extract_mesh on a coloured
 * volume (mqr_vbg_create_color) and mqr_mesh_simplify_clustering on a coloured input make them: for every
 * other producer device_colors reports a null pointer and copy_colors is status 2.
 * device_colors: the array in place, as mqr_geom_device_ptrs.  copy_colors: nv*3 float32 into `loc` memory. */
int mqr_geom_device_colors(mqr_geom* g, void** colors);
int mqr_geom_copy_colors(mqr_geom* g, float* colors, int loc);

/* build_confidence_map / compute_pixel_error_map
 * (confidence_estimation/estimate_depth_confidences.py:15-79, compute_pixel_error_map.py:120-220)
 * for reference frames [ref_begin, ref_end) of an N-frame sequence, all on the device at once.
 * depths: N*H*W float32 metric; K: N*9, T_cw: N*16, T_cw_inv: N*16 float32 (host);
 * frame_ok: N bytes (host, may be NULL).  conf: (ref_end-ref_begin)*H*W float64,
 * valid: same int32, both in `out_loc` memory.  float64 arithmetic as numpy does it. */
int mqr_confidence(int device, const float* depths, int depth_loc, int N, int H, int W, const float* K,
                   const float* T_cw, const float* T_cw_inv, const uint8_t* frame_ok, int ref_begin, int ref_end,
                   int frame_range, double depth_max, double error_threshold, double* conf, int32_t* valid,
                   int out_loc);
/* mqr_confidence for host output as two bytes per pixel: counts[r][y][x] = valid_count | consistent_count
 * << 8 of reference frame ref_begin + r (csrc/confpack.hip: the maps computed into HBM, reduced on the device,
 * each pair checked to give back the map's exact float64 bits; 2 bytes cross the link instead of 12).
 * *packed = 1 on success; 0 when a pixel does not fit (more than 255 valid neighbours) -- counts is then
 * unspecified and the caller uses mqr_confidence.  The pairs expand to the maps in
 * mqr_write_confidence_npz_counts. */
int mqr_confidence_counts(int device, const float* depths, int depth_loc, int N, int H, int W, const float* K,
                          const float* T_cw, const float* T_cw_inv, const uint8_t* frame_ok, int ref_begin,
                          int ref_end, int frame_range, double depth_max, double error_threshold, uint16_t* counts,
                          int* packed);
/* Diagnostic: enable (1) / disable (0) / keep (-1) per-pair stage counting of mqr_confidence on this
 * device (a slower kernel build).  4 = counting off and the branchy float32 prefilter stages forced: they
 * are the path of frames whose byte offsets do not fit 32 bits, and this is the test hook that runs them
 * on small frames (identical maps); 0 or 1 returns to the default stages.  Any other value is an error.
 * last4 (nullable) = the last counted call's (pixel, neighbour) pairs with a valid reference pixel, and how
 * many the float32 prefilter, the float64 band filter and the float64 back-projection decided. */
int mqr_confidence_stats(int device, int enable, int64_t* last4);
int mqr_pixel_error_map(int device, const float* ref_depth, const float* tgt_depth, int H, int W, const float* K_ref,
                        const float* K_tgt, const float* T_cw_ref, const float* T_cw_inv_tgt, const float* T_cw_tgt,
                        double depth_max, float* err_out);

/* Device-side depth ingestion.  N raw Quest NDC buffers (H*W float32, raw_loc
 * MQR_HOST / MQR_DEVICE) -> metric depth (depth_out, out_loc) + per-frame validity frame_ok[N]
 * (host).  Replaces DepthDataIO.load_depth_map + is_depth_map_valid
 * (scripts/dataio/depth_data_io.py:33-53, 80-85), convert_depth_to_linear
 * (scripts/utils/depth_utils.py:21-46) and the confidence mask of load_depth_map
 * (processing/reconstruction/utils/o3d_utils.py:131-142).  strong[f] (nullable): bit 0 / bit 1 =
 * near / far were numpy float64 scalars (numpy >= 2 then divides in float64; Python floats keep
 * the decode in float32).  has_mask[f] (nullable) selects frames whose conf (float64) /
 * valid_count (int32) maps, laid out like the depth, are applied: depth = 0 where
 * conf < conf_thr or valid_count < count_thr. */
int mqr_decode_depth(int device, const float* raw, int raw_loc, int N, int H, int W, const double* nears,
                     const double* fars, const uint8_t* strong, const double* conf, const int32_t* valid_count,
                     const uint8_t* has_mask, int mask_loc, double conf_thr, int count_thr, float* depth_out,
                     int out_loc, uint8_t* frame_ok);
/* The same decode with the confidence mask given as one byte per pixel (mask[N][H][W], mask_loc; nonzero =
 * depth 0 where has_mask[f]), e.g. as mqr_read_frames_masked computes it from the npz: 1 byte per pixel to
 * stage instead of 12. */
int mqr_decode_depth_masked(int device, const float* raw, int raw_loc, int N, int H, int W, const double* nears,
                            const double* fars, const uint8_t* strong, const uint8_t* mask, const uint8_t* has_mask,
                            int mask_loc, float* depth_out, int out_loc, uint8_t* frame_ok);

/* Device-side colour-frame ingestion (csrc/colorframes.hip).  N raw Quest camera frames (Android
 * YUV_420_888, raw_loc MQR_HOST / MQR_DEVICE, frame f at raw + f * frame_stride; the stride and the bases
 * need no alignment) -> rgb_out[N][H][W][3] uint8 (out_loc), R,G,B per pixel, or B,G,R when bgr != 0.
 * Replaces convert_yuv420_888_to_bgr (scripts/utils/image_utils.py:6-71) per frame; the colour arithmetic
 * restates OpenCV's as recalled (csrc/color_convert.hpp: parity unpinned).  W and H are even.  The plane
 * layout is resolved by the caller (mqr/colorframes.py resolve_layout): byte (row, col) of a plane is at
 * base + row * row_stride + col * step of its frame; Y has H x W of them, U and V H/2 x W/2.  Every such byte
 * must lie below valid_bytes (checked before launch; nothing past it is read).
 * Optional per-frame statistics of the decoded image, host arrays, computed only when non-null:
 *   hist[N][256]     exact histogram of the blue channel;
 *   lap_sums[N][2]   the exact sums of x and of x*x over the 3x3 Laplacian (ksize 1, border reflect-101) of
 *                    the integer grey image. */
typedef struct mqr_yuv_layout {
    int64_t y_base, y_row_stride, y_pixel_stride;
    int64_t u_base, u_row_stride, u_step;
    int64_t v_base, v_row_stride, v_step;
    int64_t valid_bytes;
} mqr_yuv_layout;
int mqr_decode_color_frames(int device, const uint8_t* raw, int raw_loc, int N, int64_t frame_stride, int W, int H,
                            const mqr_yuv_layout* layout, int bgr, uint8_t* rgb_out, int out_loc, uint32_t* hist,
                            int64_t* lap_sums);
/* Device time of the last completed mqr_decode_color_frames call on `device`, from events around its
 * kernels: the decode kernel, and the statistics pass with its memset (0 when no statistics were asked for). */
int mqr_color_frames_last_ms(int device, float* decode_ms, float* stats_ms);
/* The integer constants of that arithmetic, in the order CY, CUB, CUG, CVG, CVR, shift, grey B, grey G,
 * grey R, grey shift (csrc/color_convert.hpp is their one home; the host path reads them from here). */
#define MQR_COLOR_CONSTANTS 10
int mqr_color_constants(int32_t* out, int n);

/* Host reads of the drop-in integrate.  Replaces, for n frames, the raw depth
 * read of DepthDataIO.load_depth_map (np.fromfile of H*W little-endian float32,
 * scripts/dataio/depth_data_io.py:33-53) and load_confidence_map (np.load of the np.savez npz:
 * confidence_map <f8 HxW, valid_count <i4 HxW; depth_data_io.py:91-104): `threads` native threads pread
 * the files straight into raw_out[n][H][W] and, when conf_paths is non-null, conf_out / vc_out[n][H][W]
 * (conf_paths[f] may be null: no confidence read for that frame).  Host-only (no device work).
 * status[f] is a set of MQR_FRAME_* bits.  A missing or unreadable raw file leaves zeros in raw_out
 * (decoded invalid); *_OTHER (wrong size, a compressed / non-standard npz, another dtype or shape, a read
 * error) is left to the caller's own loader, which then raises or logs exactly as the reference does. */
#define MQR_FRAME_RAW_OK 1
#define MQR_FRAME_RAW_MISSING 2
#define MQR_FRAME_RAW_OTHER 4
#define MQR_FRAME_CONF_OK 8
#define MQR_FRAME_CONF_MISSING 16
#define MQR_FRAME_CONF_OTHER 32
int mqr_read_frames(int n, const char* const* raw_paths, const char* const* conf_paths, int H, int W,
                    float* raw_out, double* conf_out, int32_t* vc_out, uint8_t* status, int threads);
/* The same reads with the confidence maps reduced while they are read to the mask byte the decode applies:
 * mask_out[f][y][x] = (confidence_map < conf_thr) | (valid_count < count_thr) (o3d_utils.py:131-142),
 * for mqr_decode_depth_masked. */
int mqr_read_frames_masked(int n, const char* const* raw_paths, const char* const* conf_paths, int H, int W,
                           double conf_thr, int count_thr, float* raw_out, uint8_t* mask_out, uint8_t* status,
                           int threads);

/* The confidence maps' writer (SURVEY §8 C3 outputs): for n frames, np.savez(paths[f],
 * confidence_map=conf[f], valid_count=valid[f]) as the reference saves them
 * (scripts/dataio/depth_data_io.py:106-115) -- a zip of stored members confidence_map.npy (<f8 H x W) and
 * valid_count.npy (<i4 H x W), .npy format 1.0 headers, zip64 local extra fields and CRC-32 like
 * np.savez's -- written by `threads` native threads from the caller's arrays.  Host-only.
 * paths[f] may be null (no file for that frame).  status[f]: 0, or the errno of the failed open / write
 * (the caller reports that frame). */
int mqr_write_confidence_npz(int n, const char* const* paths, const double* conf, const int32_t* valid, int H, int W,
                             int32_t* status, int threads);
/* The same files from the confidence maps' two counts per pixel: counts[f][y][x] = valid_count |
 * consistent_count << 8 (as mqr_confidence_counts downloads them); confidence_map = consistent / valid in
 * float64, 0 where valid is 0 (estimate_depth_confidences.py:72-74), expanded by the writer threads. */
int mqr_write_confidence_npz_counts(int n, const char* const* paths, const uint16_t* counts, int H, int W,
                                    int32_t* status, int threads);
/* CRC-32 (zip / zlib) of len bytes continuing from crc (0 to start): the writer's checksum, exported for
 * its tests. */
uint32_t mqr_crc32(uint32_t crc, const void* data, int64_t len);

/* Kernel timing (HIP events on the volume's own stream).  enable=1 starts recording every
 * integrate-kernel launch; stats: launches, total kernel ms, union blocks, frame-blocks
 * (sum of per-frame touched blocks), frames, and the same for touch. */
typedef struct mqr_stats {
    int64_t integrate_launches;
    double integrate_ms;
    int64_t union_blocks;
    int64_t frame_blocks;
    int64_t frames;
    int64_t touch_launches;
    double touch_ms;
    int64_t pixels;
    int64_t table_retries; /* batches touched again after the probe-limited table filled up */
} mqr_stats;
/* enable: 0 off, 1 time every integrate launch (two events per batch on the integrate stream), 2 also
 * every touch launch (two more on the touch stream); results in mqr_vbg_stats. */
int mqr_vbg_profile(mqr_vbg* v, int enable);

/* Test hooks.  mqr_vbg_set_variant: low byte = integrate kernel (0 default = the fast kernels where their
 * preconditions hold, 1 generic, 2 exact R-specialised, 4 lean with dword gathers; all bit-identical, see
 * launch_integrate in csrc/vbg.hip).  Three bits each force a path that some input selects on its own, so
 * that a test can reach it with ordinary frames:
 *   bit 12  the batch touch probes one table slot per new key: the full-table undo-and-retry path (a batch
 *           that fills the probe-limited table);
 *   bit 26  k_integrate_win instead of the LDS-table kernel k_integrate_wt (a volume whose weight bound is
 *           unknown, or above the table's capacity);
 *   bit 27  k_integrate_wt keeps two Markstein corrections of s / sdf_trunc (an sdf_trunc for which one
 *           correction is not verified exact).
 * Every other value -- another low byte, or any other bit: the driver modes measured and retired, DESIGN.md
 * §4.1 -- is rejected: non-zero return, mqr_last_error set, the volume's configuration left as it was.
 * mqr_check_division: exhaustive bit-pattern check of the division shortcuts used on device against
 * IEEE division (which=0: 1/b via rcp_rn, 1: a/b via div_rn, 2: a/b via the bare core, 3: 1/b via
 * rcp_nm, 4: 1/b via rcp_m, over float bit patterns [lo_bits, lo_bits+count) as b or a); returns
 * the mismatch count and the first bad pattern. */
int mqr_vbg_set_variant(mqr_vbg* v, int variant);
int mqr_check_division(int device, int which, float b, uint32_t lo_bits, uint64_t count, uint32_t* mismatches,
                       uint32_t* first_bad);
/* mqr_check_div64: the confidence kernel's float64 quotients against IEEE division on `count`
 * hashed pairs (a in [-a_max, a_max], b log-uniform in [b_lo, b_hi]); mode 0 = shared refined
 * reciprocal (quotients by Z), 1 = host-rounded reciprocal + Markstein correction (by fx / fy).
 * first_bad: 2 doubles (a, b) of a mismatch. */
int mqr_check_div64(int device, int mode, uint64_t seed, uint64_t count, double a_max, double b_lo, double b_hi,
                    uint64_t* mismatches, double* first_bad);
int mqr_vbg_stats(mqr_vbg* v, mqr_stats* out, int reset);

/* Ray casting: replaces o3d.t.geometry.RaycastingScene as used for colour-aligned
 * depth (reconstruct_scene.py:197-201, o3d_utils.py:324-341, optimize_color_pose.py:24-47).
 * add_triangles ~ RaycastingScene.add_triangles (vertices float32 (nv,3), triangles int32 (nt,3),
 * loc MQR_HOST/MQR_DEVICE; returns the geometry id); the device BVH is (re)built on the first
 * query after a change (mqr_scene_build forces it).  cast_pinhole ~ create_rays_pinhole(K, T_wc,
 * W, H) + cast_rays for n_frames cameras (K (n,3,3) and T_wc (n,4,4) float64 row-major);
 * cast_rays takes explicit rays (n,6) float32 (origin, direction).  Outputs: t_hit (inf on miss)
 * and the optional geometry / primitive ids (0xffffffff on miss), barycentric uvs (n,2) and unit
 * geometric normals (n,3); out_loc says where all output buffers live. */
/* Per-vertex colour from keyframes: the colour averaging of Open3D's
 * colour-map pipeline fed by the reference (optimize_color_pose.py:24-73 -> run_rigid_optimizer;
 * upstream ColorMapUtils.cpp CreateVertexAndImageVisibility + SetGeometryColorAverage, VERIFY).
 * vertices nv*3 float32; images N*H*W*3 uint8 RGB; depths N*H*W float32 colour-aligned depth
 * (ray-cast, raycast_in_color_view); K N*9, T_wc N*16 float64 host.  colors_out nv*3 float32 in
 * [0, 1] (0 where no keyframe sees the vertex), counts_out nv int32 (nullable).  Open3D defaults:
 * max_depth 2.5, visibility_threshold 0.03, margin 10. */
int mqr_color_vertices(int device, const float* vertices, int64_t nv, int vertices_loc, const uint8_t* images,
                       const float* depths, int images_loc, int N, int H, int W, const double* K, const double* T_wc,
                       double max_depth, double visibility_threshold, int margin, float* colors_out,
                       int32_t* counts_out, int out_loc);
/* mqr_color_map: the complete vertex colouring of run_rigid_optimizer with the keyframe poses as
 * given (optimize_color_pose.py:70-73 at maximum_iteration = 0; the refinement: mqr_colormap_*): t_hit = raycast_in_color_view
 * depth (o3d_utils.py:324-341), RGBD depth truncated at depth_trunc (3.0), depth-discontinuity
 * masks (Sobel magnitude > disc_threshold 0.1, dilated by half_dilation 3), visibility, float64
 * colour means, and vertices no keyframe samples filled with the mean of their knn (3) nearest
 * sampled vertices.  counts: keyframes averaged (0 for filled vertices). */
int mqr_color_map(int device, const float* vertices, int64_t nv, int vloc, const uint8_t* images, const float* t_hit,
                  int img_loc, int N, int H, int W, const double* K, const double* T_wc, double max_depth,
                  double visibility_threshold, int margin, double disc_threshold, int half_dilation, double depth_trunc,
                  int knn, float* colors_out, int32_t* counts_out, int out_loc);

int mqr_scene_create(int device, mqr_scene** out);
int mqr_scene_destroy(mqr_scene* s);
int mqr_scene_add_triangles(mqr_scene* s, const float* vertices, int64_t nv, const int32_t* triangles, int64_t nt,
                            int loc, uint32_t* geom_id);
int mqr_scene_build(mqr_scene* s);
int mqr_scene_triangle_count(mqr_scene* s, int64_t* n);
int mqr_scene_cast_pinhole(mqr_scene* s, const double* K, const double* T_wc, int n_frames, int H, int W,
                           float* t_hit, uint32_t* geom_ids, uint32_t* prim_ids, float* uvs, float* normals,
                           int out_loc);
int mqr_scene_cast_rays(mqr_scene* s, const float* rays, int64_t nrays, int rays_loc, float* t_hit,
                        uint32_t* geom_ids, uint32_t* prim_ids, float* uvs, float* normals, int out_loc);

/* filter_mesh_components (processing/reconstruction/utils/o3d_utils.py:241-321) on the device:
 * edge-connected triangle clusters (Open3D cluster_connected_triangles order), keep clusters with
 * >= min_triangle_count triangles (else the largest), then remove_unreferenced_vertices,
 * remove_degenerate_triangles, remove_duplicated_triangles, remove_duplicated_vertices and
 * remove_non_manifold_edges with Open3D's legacy semantics (non-manifold edges visited in
 * ascending vertex-pair order).  vertices / normals (nullable) nv*3 float32, triangles nt*3 int32
 * in `loc` memory.  Result: a device geometry (mqr_geom_counts / _copy / _free).  stats[8]:
 * input triangles, clusters, kept clusters, triangles removed with small clusters, largest
 * cluster, triangles removed by the non-manifold pass, final triangles, final vertices. */
int mqr_mesh_filter_components(int device, const float* vertices, const float* normals, int64_t nv,
                               const int32_t* triangles, int64_t nt, int loc, int64_t min_triangle_count,
                               mqr_geom** out, int64_t* stats);

/* compute_raw_metrics_for_mesh (scripts/evaluation/evaluate_fbx_quality.py:253-441) on the device: the
 * reference's raw quality metrics of one triangle mesh -- triangle shape, edge topology, vertex-graph
 * components, vertex-normal deviation and dihedral statistics, the 10^3 vertex-density grid and the
 * colour gradient -- in float64 on float32 inputs.  The fields are RawMeshMetrics' after name / path,
 * in its order; booleans are 0 / 1.  vertices nv*3 float32, colors nullable nv*3 float32 in [0, 1],
 * triangles nt*3 int32, all in `loc` memory (MQR_DEVICE buffers are read in place).  Errors: nv == 0
 * or nt == 0 (the reference raises ValueError), 3 nt >= 2^31, a non-finite coordinate, a triangle
 * index outside [0, nv) (found by a kernel that reads only the indices, before any gather). */
typedef struct mqr_quality_metrics {
    double mean_aspect_ratio;
    double mean_skewness;
    int64_t degenerate_triangles;
    int64_t non_manifold_edges;
    double boundary_edge_ratio;
    int64_t component_count;
    int64_t total_edges;
    double normal_deviation_avg_deg;
    double dihedral_min_deg;
    double dihedral_max_deg;
    double dihedral_penalty;
    double surface_roughness;
    int64_t is_single_component;
    double vertex_density_stddev;
    int64_t has_color;
    double uncolored_vertex_ratio;
    double color_gradient_stddev;
    int64_t is_manifold;
    int64_t is_watertight;
    int64_t num_vertices;
    int64_t num_triangles;
} mqr_quality_metrics;
int mqr_mesh_quality(int device, const float* vertices, int64_t nv, const float* colors, const int32_t* triangles,
                     int64_t nt, int loc, mqr_quality_metrics* out);

/* ---- ground-truth comparison (analysis/computation/compare_mesh_to_ground_truth.py) -----------------
 * The three device primitives behind mqr.compare_mesh_to_ground_truth (rules in DESIGN §2.6).
 *
 * Nearest neighbour (Open3D compute_point_cloud_distance, KDTreeFlann.search_knn_vector_3d with k = 1).
 * create: a search tree over n float32 xyz targets in `loc` memory.  The tree keeps its own Morton-ordered
 * copy: the caller's buffer (MQR_DEVICE buffers are read in place) is free again on return.  Errors:
 * n == 0, n >= 2^31, a coordinate that is not finite or beyond 1e18 in magnitude (found by a kernel that
 * reads but never gathers; within that range the float32 bounds the search prunes on cannot overflow,
 * which the exactness below depends on).
 * query: for each of nq float32 xyz queries in `loc` memory the nearest target: dist[i] float64 and
 * idx[i] int32 (idx may be NULL), in `out_loc` memory.  Rule: d2 = (dx*dx + dy*dy) + dz*dz in float64 on
 * the widened float32 coordinates, without contraction; dist = sqrt(d2); among targets of equal d2 the
 * lowest index wins.  The result is exact (a brute-force search gives the same bits) and independent of
 * the order of the queries.  nq == 0 is a no-op; nq >= 2^31 or a query coordinate that is not finite or
 * beyond 1e18 in magnitude is an error. */
typedef struct mqr_nn mqr_nn;
int mqr_nn_create(int device, const float* targets, int64_t n, int loc, mqr_nn** out);
int mqr_nn_query(mqr_nn* h, const float* queries, int64_t nq, int loc, double* dist, int32_t* idx, int out_loc);
int mqr_nn_destroy(mqr_nn* h);

/* np.mean, np.std (population, two passes), np.min, np.max, np.median and (dist < threshold).sum() of n
 * non-negative finite float64 values in `loc` memory; only the struct crosses to the host.  Sums run in a
 * fixed order, so a repeated call is bit-identical; the median comes from a radix sort of the bit patterns
 * (an even count gives the mean of the two middle values).  Errors: n == 0, n >= 2^31. */
typedef struct mqr_distance_stats_result {
    double mean;
    double std;
    double min;
    double max;
    double median;
    int64_t count_below; /* values < threshold, strict */
    int64_t count;       /* n */
} mqr_distance_stats_result;
int mqr_distance_stats(int device, const double* dist, int64_t n, int loc, double threshold,
                       mqr_distance_stats_result* out);

/* One mesh's measures on one edge sort: vertices nv*3 float32, triangles nt*3 int32 in `loc` memory
 * (MQR_DEVICE buffers are read in place), all arithmetic float64 on the float32 inputs in a fixed order.
 *   surface_area   sum of 0.5 |(p1 - p0) x (p2 - p0)| (get_surface_area);
 *   min / max      the axis-aligned bounds, exact;
 *   volume         |sum of p0 . (p1 x p2) / 6| when is_closed_oriented, else 0.0 (the reference catches
 *                  Open3D's "not watertight" exception and uses 0.0);
 *   is_closed_oriented  every edge (loop edges of degenerate triangles included) lies on exactly two
 *                  triangles that traverse it in opposite directions.  DEVIATION: Open3D's get_volume also
 *                  refuses vertex-non-manifold and self-intersecting meshes; this pass does not test for
 *                  either, and reports their signed sum;
 *   boundary_edges the edges that lie on exactly one triangle.
 * `boundary` (may be NULL) receives those edges as (min, max) vertex pairs, ascending by their slot
 * 3 t + e (edge e of triangle t: the order in which the reference's dictionary first meets them), kept in
 * HBM: mqr_edge_list_count / _copy (2 n int32 into `loc` memory) / _free.  It stays NULL when there are
 * none.  nt == 0 is allowed: area 0, volume 0, no boundary.  Errors: nv == 0, 3 nt >= 2^31, a non-finite
 * coordinate, a triangle index outside [0, nv) (found before any gather). */
typedef struct mqr_mesh_measure_result {
    double surface_area;
    double volume;
    double min_bound[3];
    double max_bound[3];
    int64_t is_closed_oriented;
    int64_t boundary_edges;
    int64_t num_vertices;
    int64_t num_triangles;
} mqr_mesh_measure_result;
typedef struct mqr_edge_list mqr_edge_list;
int mqr_mesh_measure(int device, const float* vertices, int64_t nv, const int32_t* triangles, int64_t nt, int loc,
                     mqr_mesh_measure_result* out, mqr_edge_list** boundary);
int mqr_edge_list_count(mqr_edge_list* list, int64_t* n);
int mqr_edge_list_copy(mqr_edge_list* list, int32_t* pairs, int loc);
int mqr_edge_list_free(mqr_edge_list* list);

/* ---- surface samples (TriangleMesh.sample_points_uniformly, reconstruct_scene.py:151-171) ------------
 * n area-weighted samples of a mesh's surface (csrc/meshsample.hip; the rule is this package's own, DESIGN
 * §2.8: Open3D draws from std::mt19937, which is not matched).  vertices nv*3 float32, normals / colors
 * nullable nv*3 float32, triangles nt*3 int32, all in `in_loc` memory (MQR_DEVICE buffers are read in place);
 * out_positions n*3 float32 and the nullable out_normals / out_colors (n*3 float32) and out_triangle (n int32:
 * the triangle each sample lies on), all in `out_loc` memory.  Sample i is a function of (mesh, seed, i)
 * alone: a repeated call, another n, and host or device residency give identical bits.  Triangles are drawn
 * in proportion to integer weights floor(area 2^(32 - e)) (largest area = m 2^e, m in [0.5, 1)), so a
 * triangle below 2^-32 of the largest has weight 0 and is never drawn; the point is (wa a + wb b) + wc c in
 * float64 with (wa, wb, wc) = (1 - s, s (1 - u2), s u2), s = sqrt(u1), rounded to float32; normals and colours
 * take the same weights and are not renormalised; with use_triangle_normal the normal is the drawn triangle's
 * unit normal instead (the vertex normals are then not read).  out_normals needs normals or
 * use_triangle_normal, out_colors needs colors.  The work runs on the calling thread's caller stream
 * (mqr_set_stream) and is complete on return.  n == 0 is a no-op.  Errors: nt == 0, n < 0, nt or nv >= 2^31,
 * a non-finite coordinate, a triangle index outside [0, nv) (both found before any gather), every triangle
 * degenerate (total weight zero; the outputs are then not written). */
int mqr_mesh_sample_points(int device, const float* vertices, int64_t nv, const float* normals, const float* colors,
                           const int32_t* triangles, int64_t nt, int in_loc, int64_t n, uint64_t seed,
                           int use_triangle_normal, float* out_positions, float* out_normals, float* out_colors,
                           int32_t* out_triangle, int out_loc);
/* The two entries below are measurement hooks for tools/mesh_sample_probe.py, not for production callers
 * (as mqr_color_frames_last_ms and mqr_vbg_set_variant are).
 * last_ms: device time of the last completed call on `device`, ms, by events on the stream it ran on: the
 * whole call (input checks and their host read included), the selection table (areas, weights, scan, coarse
 * table), and the sample kernel.
 * set_flat_search: non-zero makes the sample kernel search the whole prefix-sum table instead of the coarse
 * table and one segment.  The samples are identical either way.  The setting is process-wide (an atomic
 * word, read once by each call). */
int mqr_mesh_sample_last_ms(int device, float* call_ms, float* table_ms, float* sample_ms);
int mqr_mesh_sample_set_flat_search(int flat);

/* ---- mesh simplification by vertex clustering (scripts/downsample_fbx_mesh.py:129-283) ---------------
 * mesh.simplify_vertex_clustering(voxel_size, Average) (csrc/meshsimplify.hip).  The rule is restated from
 * Open3D's SimplifyVertexClustering as recalled (unpinned; where Open3D's result follows the
 * iteration order of its hash containers the order is this package's own).  Quadric decimation is NOT here.
 * vertices nv*3 float32, normals / colors nullable nv*3 float32, triangles nt*3 int32 (NULL with nt == 0), all
 * in `loc` memory (MQR_DEVICE buffers are read in place).  All arithmetic is float64 on the widened values:
 *   origin = (double)min_bound - voxel_size * 0.5 and cell(i) = floor(((double)p_i - origin) / voxel_size),
 *   per axis; output vertex j is the j-th distinct cell in order of first appearance over i = 0 .. nv - 1 and
 *   map[i] = j; its position is the members' sum in ascending input index (from +0), divided by (double)count
 *   and rounded to float32; normals and colours likewise, neither renormalised nor clamped (without input
 *   normals the result's normals are zeros; without input colours it has none).  Triangles in input order:
 *   (a, b, c) = map[corners]; dropped when two are equal; rotated cyclically so the smallest index comes first
 *   (the orientation stays); dropped when the same rotated triple occurred at a lower input index.  The same
 *   cells in the opposite orientation are another triple: both stay.
 * The result equals that rule bit for bit, whatever the residency, and a repeated call is identical.
 * vertex_bounds: the exact bounds of the float32 coordinates as doubles (a -0 reads +0).
 * mesh_cluster_count: the output vertex count of a voxel size (bounds, keys, one sort, segment heads; nothing
 *   else is computed or written).
 * mesh_simplify_clustering: the result is a device geometry from the block pool (mqr_geom_counts / _copy /
 *   _device_ptrs / _device_colors / _copy_colors / _free).  stats[8]: input vertices, output vertices, input
 *   triangles, triangles dropped as collapsed, triangles dropped as duplicates, output triangles, the largest
 *   cell's population, the largest cell count along an axis.
 * Errors (status 2; *out stays NULL): voxel_size not finite or <= 0, nv == 0, nv or nt >= 2^31, a non-finite
 * coordinate, a triangle index outside [0, nv) (both found before any gather), and a grid of 2^21 or more
 * cells along an axis ("the grid is too fine"; DEVIATION: Open3D's limit is INT_MAX cells -- the tighter one
 * makes the cell key one 63-bit word).  The work runs on the calling thread's caller stream (mqr_set_stream)
 * and is complete on return. */
int mqr_vertex_bounds(int device, const float* vertices, int64_t nv, int loc, double* min3, double* max3);
int mqr_mesh_cluster_count(int device, const float* vertices, int64_t nv, int loc, double voxel_size,
                           int64_t* n_cells);
int mqr_mesh_simplify_clustering(int device, const float* vertices, int64_t nv, const float* normals,
                                 const float* colors, const int32_t* triangles, int64_t nt, int loc, double voxel_size,
                                 mqr_geom** out, int64_t* stats);
/* A measurement hook for tools/mesh_simplify_probe.py (as mqr_mesh_sample_last_ms): device time of the last
 * completed mqr_mesh_simplify_clustering or mqr_mesh_cluster_count on `device`, ms, by events on the stream it
 * ran on, from behind the input copies to the last kernel (the host's reads of the check flags and the cell
 * count included): the whole call, the part up to the output vertices, and the triangles (0 for a count). */
int mqr_mesh_simplify_last_ms(int device, float* call_ms, float* vertex_ms, float* triangle_ms);

/* Fragment registration (refine_fragment_poses.py:122-271): a CLOUD SET of N float32 xyz clouds in
 * HBM and three batched operations over pairs of them, standing in for Open3D's
 * evaluate_registration, multi_scale_icp (point to point) and get_information_matrix.
 * create: points[i] -> counts[i] x 3 float32, all in `loc` memory.  MQR_HOST clouds are copied;
 * MQR_DEVICE clouds are used IN PLACE (no copy): the caller keeps them allocated and unchanged until
 * mqr_cloudset_destroy.  Fails on an empty cloud or a non-finite coordinate.  The set caches, per
 * cloud, each point selection asked for (full, every k-th point, voxel down-sample at v) and a
 * uniform-grid index per (selection, search radius); a coordinate whose cell index would pass 2^20
 * per axis fails the call that needs the view.
 * voxel_down: the down-sampled view of one cloud (key floor(p / v) per axis in float64, members
 * summed in ascending original index in float64, output in ascending (kx, ky, kz) order); *n
 * receives the point count, `out` (may be NULL to ask for the count only) n x 3 float32 in `loc`.
 * Pairs: src[p], tgt[p] index the set's clouds; T row-major 4x4 float64 per pair (source to target).
 * evaluate_pairs: fitness = correspondences / source points and inlier rmse of T, on every k-th
 * point of both clouds (every_k <= 1: all points).
 * icp_pairs: per level l both clouds voxel down-sampled at voxel_sizes[l] (<= 0: the full cloud),
 * up to max_iters[l] point-to-point iterations at max_dists[l] with Open3D's relative fitness / rmse
 * stopping rule; T_out, fitness, rmse of the last level; iterations[p * n_levels + l] = the
 * correspondence passes pair p ran on level l.
 * information_pairs: Open3D's 6x6 information matrix of T over the FULL clouds, info[36] per pair.
 * Results are deterministic: a repeated call, alone or in any batch, is bit-identical. */
typedef struct mqr_cloudset mqr_cloudset;
int mqr_cloudset_create(int device, int n_clouds, const float* const* points, const int64_t* counts, int loc,
                        mqr_cloudset** out);
int mqr_cloudset_destroy(mqr_cloudset* set);
int mqr_cloudset_voxel_down(mqr_cloudset* set, int cloud, double voxel_size, int64_t* n, float* out, int loc);
int mqr_evaluate_pairs(mqr_cloudset* set, int n_pairs, const int32_t* src, const int32_t* tgt, int every_k,
                       double max_dist, const double* T, double* fitness, double* rmse, int64_t* ncorr);
int mqr_icp_pairs(mqr_cloudset* set, int n_pairs, const int32_t* src, const int32_t* tgt, int n_levels,
                  const double* voxel_sizes, const double* max_dists, const int32_t* max_iters,
                  const double* rel_fitness, const double* rel_rmse, const double* T_init, double* T_out,
                  double* fitness, double* rmse, int32_t* iterations);
int mqr_information_pairs(mqr_cloudset* set, int n_pairs, const int32_t* src, const int32_t* tgt, double max_dist,
                          const double* T, double* info);

/* ---- odometry information (make_fragments.py:106-240) -------------------------------------------
 * o3d.t.pipelines.odometry.compute_odometry_information_matrix for n_pairs image pairs of one stack of
 * N metric float32 depth frames (H x W each, host or device by depth_loc) in one launch.  K: the 3x3
 * intrinsic matrix shared by the frames; T: n_pairs 4x4 transforms, source camera -> target camera
 * (host float64).  info (host): n_pairs 6x6 float64 in the order (rx, ry, rz, tx, ty, tz); counts (host,
 * may be NULL): the accepted pixels of each pair.  Float64 rules and a fixed summation order (DESIGN
 * "odometry information rules"): a repeated call, and a pair alone or inside a batch, give identical
 * bits.  The work runs on the calling thread's caller stream (mqr_set_stream) and the call returns with
 * the host outputs filled.  n_pairs == 0 is a no-op; an index outside [0, N), a non-finite K or T or
 * a non-positive N, H or W is status 2 before anything is launched.  The library keeps its device
 * scratch (pairs, partial sums, results and, for MQR_HOST frames, a copy of the frame stack) per device
 * for the life of the process, grow-only; there is no entry that releases it. */
int mqr_odometry_information_pairs(int device, const float* depths, int depth_loc, int N, int H, int W,
                                   const double* K, int n_pairs, const int32_t* src, const int32_t* tgt,
                                   const double* T, double dist_threshold, double depth_scale, double depth_max,
                                   double* info, int64_t* counts);

/* ---- colour-map optimisation (optimize_color_pose.py:70-73) --------------------------------------
 * o3d.pipelines.color_map.run_rigid_optimizer, device resident from start to finish (the
 * rules, restated from Open3D 0.19 as recalled).  A handle holds the vertices, the keyframes' utility
 * images (grey, d/dx, d/dy), the depth-boundary masks' outcome -- both visibility lists, computed once
 * at the poses given to create -- and the current poses, all in HBM.
 * create: arguments as mqr_color_map (vertices nv*3 float32 by vloc; images N*H*W*3 uint8 and t_hit
 *   N*H*W float32 by iloc; K N*9, T_wc N*16 float64 host).  MQR_DEVICE vertices and images are used in
 *   place and must stay valid and unchanged until destroy; t_hit is only read by create.  H, W >= 2,
 *   margin >= 0, N <= 65535.  A non-finite K or T_wc is status 2 ("non-finite").  N == 0 or nv == 0
 *   gives a handle that touches no device: every call on it succeeds and reports zeros.
 * counts: the visibility pairs of each keyframe (N int64, host).
 * set_poses / get_poses: N*16 float64 host, world -> camera.  The visibility lists stay as created.
 * proxy: recomputes every vertex's proxy intensity at the current poses; proxy (nv float64, host) may
 *   be NULL.
 * systems: one evaluation at the current poses and proxies, no update: JTJ N*36 (symmetric), JTr N*6,
 *   r2 N, count N (host).  Proxies older than the last set_poses are recomputed first.
 * optimize: max_iteration iterations of (all systems, all pose updates, proxies) enqueued back to back;
 *   residuals[it] = the sum of the keyframes' r2 and counts[it] = their terms in iteration it (host,
 *   read once at the end).  max_iteration == 0 is a no-op.
 * colors: the float64 mean colours over the visibility pairs at the current poses, then mqr_color_map's
 *   fill of unsampled vertices from their knn (0..8) nearest sampled ones; colors nv*3 float32 and
 *   counts nv int32 (may be NULL) by loc.  With the poses as created it is bit-identical to
 *   mqr_color_map.
 * Every sum has a fixed order (no float atomics): repeated runs are bit-identical.  A handle serves one
 * thread at a time. */
typedef struct mqr_colormap mqr_colormap;
int mqr_colormap_create(int device, const float* vertices, int64_t nv, int vloc, const uint8_t* images,
                        const float* t_hit, int iloc, int N, int H, int W, const double* K, const double* T_wc,
                        double max_depth, double visibility_threshold, int margin, double disc_threshold,
                        int half_dilation, double depth_trunc, mqr_colormap** out);
int mqr_colormap_counts(mqr_colormap* h, int64_t* pairs_per_keyframe);
int mqr_colormap_set_poses(mqr_colormap* h, const double* T_wc);
int mqr_colormap_get_poses(mqr_colormap* h, double* T_wc);
int mqr_colormap_proxy(mqr_colormap* h, double* proxy);
int mqr_colormap_systems(mqr_colormap* h, double* JTJ, double* JTr, double* r2, int64_t* count);
int mqr_colormap_optimize(mqr_colormap* h, int max_iteration, double* residuals, int64_t* counts);
int mqr_colormap_colors(mqr_colormap* h, int knn, float* colors, int32_t* counts, int loc);
/* Device time of the last optimize's launches (events on the handle's stream around the loop), ms. */
int mqr_colormap_optimize_ms(mqr_colormap* h, float* ms);
/* Hash of the colour-map optimiser's sources compiled into the library (for profile records). */
int mqr_colormap_build_tag(char* buf, int n);
int mqr_colormap_destroy(mqr_colormap* h);

/* ---- volume ray casting (csrc/volumecast.hip) --------------------------------------
 * Depth, vertex and normal maps of the fused surface for n pinhole cameras of one size, by marching each
 * pixel's ray through the block hash (Open3D's VoxelBlockGrid::RayCast surface; the rule is restated from
 * Open3D 0.19 as recalled and is not pinned against it).  K n*9 and T_wc n*16 (world -> camera) float64, host.
 * block_keys (n_keys x 3 int32 by keys_loc, or NULL = every active block) are the blocks whose projections
 * bound each ray's depth range; the march itself reads every block of the volume.  depth_min / depth_max clip
 * the range in metres; depth is t * depth_scale; pixel_offset shifts the rays within their pixels (0: the
 * pixel's corner, 0.5: its centre, the rays of mqr_scene_cast_pinhole).  flags: MQR_CAST_REFINE re-interpolates
 * the crossing from two trilinear samples where all their corners are observed.  Outputs by out_loc, each may
 * be NULL but not all: depth n*H*W, vertex and normal n*H*W*3 float32; a miss writes 0 everywhere, a normal
 * whose stencil is not wholly observed is (0, 0, 0).  The call runs behind the volume's queued integrates and
 * returns with its outputs complete.  n <= 0 or n > 65535 (a frame is one layer of the launch grid; cast more in
 * several calls), H or W <= 0, range_map_down_factor <= 0, depth_min < 0,
 * depth_max <= depth_min, a non-finite K / T_wc, fx or fy equal to 0, or all outputs NULL: status 2, nothing
 * launched.  An empty volume renders all misses. */
#define MQR_CAST_REFINE 1
int mqr_vbg_ray_cast(mqr_vbg* v, const int32_t* block_keys, int64_t n_keys, int keys_loc, const double* K,
                     const double* T_wc, int n, int H, int W, float depth_scale, float depth_min, float depth_max,
                     float weight_threshold, float trunc_voxel_multiplier, int range_map_down_factor,
                     float pixel_offset, int flags, float* depth, float* vertex, float* normal, int out_loc);
/* The same call with a colour map beside the others (nullable like them): float32 [n][H][W][3] in 0..1, the
 * colours of the 8 lattice corners around the hit vertex that exist and have weight > 0, weighted by the
 * trilinear fractions and renormalised; 0 on a miss or when no corner counts.  A colour output
 * on a volume without colour: status 2.  mqr_vbg_ray_cast is this call with color = NULL (it keeps its argument
 * list: existing callers pass 21 arguments). */
int mqr_vbg_ray_cast_color(mqr_vbg* v, const int32_t* block_keys, int64_t n_keys, int keys_loc, const double* K,
                           const double* T_wc, int n, int H, int W, float depth_scale, float depth_min,
                           float depth_max, float weight_threshold, float trunc_voxel_multiplier,
                           int range_map_down_factor, float pixel_offset, int flags, float* depth, float* vertex,
                           float* normal, float* color, int out_loc);
/* Device time (events on the volume's stream) of the last ray cast on the volume's device: the range map and
 * the march, ms. */
int mqr_vbg_ray_cast_last_ms(mqr_vbg* v, double* range_ms, double* march_ms);

#ifdef __cplusplus
}
#endif
#endif /* MQR_H */
