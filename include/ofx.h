/*
 * ofx.h — C ABI of the MI355X-native non-rigid TSDF fusion hot path (libofx.so).
 *
 * Drop-in boundary for remmel/OcclusionFusion's fusion core. Every entry point
 * takes plain device pointers + sizes and a HIP stream; no torch / numpy types
 * cross this ABI. All work is stream-ordered and asynchronous unless an entry
 * point says otherwise. Caller owns every buffer; the library owns only scratch
 * tied to an opaque handle (GN solver). Errors: int status (0 ok, <0 error) and
 * ofx_last_error() (thread-local string). Nothing throws across the ABI.
 *
 * Reference interfaces replaced (file:line in /root/reference):
 *   ofx_volume_reset        TSDFVolume.__init__ dense init tsdf=1, w=0, c=0   fusion_with_occlusion/tsdf.py:133-141
 *   ofx_volume_to_dense     TSDFVolume.get_volume (D2H on request)          tsdf.py:673-680
 *   ofx_volume_from_dense   TSDFVolume.load_volume                          tsdf.py:689-702
 *   ofx_pack_color          TSDFVolume.update colour folding                tsdf.py:545-566
 *   ofx_skin_volume_bricks  WarpField.skin_tsdf (cache build, brick cull)   warpfield.py:131-141
 *   ofx_skin_volume         WarpField.skin over TSDFVolume.world_pts       warpfield.py:83-129, tsdf.py:294-307
 *   ofx_skin_palette        (layout only) per-brick node palette of the skin_tsdf cache, warpfield.py:131-141
 *   ofx_skin_points         WarpField.skin(points, nodes)                  warpfield.py:83-129
 *                           (k-NN twin of csrc compute_pixel_anchors_euclidean, csrc/cpu/graph_proc.cpp:610-709)
 *   ofx_pack_nodes          Registration.deform_ED gathers of R, t, g       NonRigidICP/model/registration_fusion.py:168-170
 *   ofx_integrate           WarpField.deform_tsdf + TSDFVolume.integrate    warpfield.py:369-380, tsdf.py:378-494
 *                           (fused: skin cache -> ED warp -> project -> SDF/weight/colour update)
 *   ofx_integrate_palette   same, node records staged per brick in LDS      warpfield.py:369-380, tsdf.py:442-494
 *   ofx_integrate_palette_cull  same, bricks that provably update nothing skipped (per-frame cull)
 *   ofx_integrate_points    TSDFVolume.integrate of given (deformed) points  tsdf.py:442-494
 *   ofx_integrate*_w        (new) the four integrate entry points with a per-pixel observation-weight image and a cap on the
 *                           accumulated weight; ofx_observation_weights makes the image — (no reference twin: the
 *                           reference's fusion is the plain running average, tsdf.py:366-376, which stays the default.
 *                           Restated op for op by tests/weighted_ref.py)
 *   ofx_raycast             (new) depth / normal / colour images of the TSDF  — (no reference twin)
 *   ofx_deform_points       ED_warp / deform_ED / deform_mesh / normals     NonRigidICP/model/geometry.py:9-25,
 *                                                                          registration_fusion.py:157-184, warpfield.py:312-367
 *   ofx_deform_points_lbs   WarpField.deform_lbs / deform_lbs_cuda (origin form) warpfield.py:208-266,270-305
 *   ofx_visibility          TSDFVolume.check_visibility                     tsdf.py:576-612
 *   ofx_truncated_region    TSDFVolume.compute_truncated_region            tsdf.py:704-745
 *   ofx_mesh_*              measure.marching_cubes in get_mesh / get_point_cloud, colours tsdf.py:748-809
 *   ofx_backproject_depth   image_proc.backproject_depth (csrc float/ushort) utils/image_proc.py:335-349,
 *                                                                          csrc/cpu/image_proc.cpp:351-401
 *   ofx_depth_mesh_*        compute_mesh_from_depth (pixel-grid mesh)       csrc/cpu/image_proc.cpp:405-545
 *                           (EDGraph.create_mesh_from_depth, WarpField.skin of an image: embedded_deformation_graph.py:95-151,
 *                           warpfield.py:160-175)
 *   ofx_assoc_* / ofx_associate  (new) projective data association of model points with a depth frame — (no reference
 *                           twin: the reference's matches come from learned front-ends; its geometric fallback is the
 *                           truncated chamfer term, NonRigidICP/model/loss.py:275-292. Parity unpinned, as for ofx_raycast;
 *                           restated op for op by tests/assoc_ref.py)
 *   ofx_surface_*           (new) skinned surface points of the TSDF, the tracking model — (no reference twin: the
 *                           reference re-meshes and re-skins per frame, tsdf.get_deformed_model / optimizer.update in
 *                           fusion_tests/lepard_nicp_test.py:471,537. Parity unpinned; restated by tests/surface_ref.py)
 *   ofx_grow_*              (new) graph nodes added where the sampled model leaves the graph's coverage, with blended
 *                           transforms and edge rows — EDGraph.update behind WarpField.find_unreachable_nodes,
 *                           embedded_deformation_graph.py:496-609, warpfield.py:462-485 (its greedy `<` loop and 2·coverage
 *                           kept; transforms and edges have no twin. Restated op for op by tests/grow_ref.py)
 *   ofx_splat_*             (new) z-buffer of the warped model points in the live frame and the occlusion code of every
 *                           point — (no reference twin: the reference renders the live model from a warped marching-
 *                           cubes mesh, tsdf.get_deformed_model and NonRigidICP/model/point_render.py. Parity unpinned;
 *                           restated op for op by tests/splat_ref.py)
 *   ofx_prepare_depth       (new) bilateral-filtered depth of a frame, its vertex map and its normal map: what the depth
 *                           tracker reads the live frame through — (no reference twin: the reference has no depth filter.
 *                           Parity unpinned; restated op for op by tests/prepare_ref.py)
 *   ofx_photo_associate     (new) photometric correspondence search: each warped model point's best colour match in a window
 *                           of the live frame, among the pixels that pass ofx_associate's gates — (no reference twin: the
 *                           reference's dense matches come from a learned flow network. Parity unpinned; restated op for
 *                           op by tests/photo_ref.py)
 *   ofx_photo_refine        (new) sub-pixel refinement of ofx_photo_associate's matches: a translation-only inverse
 *                           compositional Lucas-Kanade step over a small colour patch, and the vertex map interpolated at
 *                           the refined pixel — (no reference twin: the reference's flow network is sub-pixel by itself.
 *                           Parity unpinned; restated op for op by tests/refine_ref.py)
 *   ofx_depth_to_pc         Registration.optimize target cloud: depth_2_pc, NonRigidICP/model/geometry.py:44-59,
 *                           mask compaction, map_pixel_to_pcd              registration_fusion.py:104-109,388-395
 *   ofx_pixel_anchors_euclidean  csrc compute_pixel_anchors_euclidean     csrc/cpu/graph_proc.cpp:610-709
 *   ofx_pixel_anchors_geodesic   csrc compute_pixel_anchors_geodesic      csrc/cpu/graph_proc.cpp:483-608
 *   ofx_remap_anchors       csrc update_pixel_anchors                       csrc/cpu/graph_proc.cpp:934-961
 *   ofx_knn_points          KDTree.query (pykdtree) in WarpField.find_unreachable_nodes  warpfield.py:462-485
 *   ofx_graph_create/destroy/adjacency  mesh vertex adjacency (std::set per vertex)  csrc/cpu/graph_proc.cpp:174-186
 *   ofx_erode_mesh          csrc erode_mesh                                 csrc/cpu/graph_proc.cpp:17-77
 *   ofx_sample_nodes        csrc sample_nodes (randomShuffle = false)       csrc/cpu/graph_proc.cpp:79-136
 *   ofx_edges_geodesic      csrc compute_edges_geodesic                     csrc/cpu/graph_proc.cpp:155-300
 *   ofx_edges_euclidean     csrc compute_edges_euclidean                    csrc/cpu/graph_proc.cpp:302-356
 *   ofx_node_edge_cleanup   csrc node_and_edge_clean_up                     csrc/cpu/graph_proc.cpp:388-438
 *   ofx_compute_clusters    csrc compute_clusters                           csrc/cpu/graph_proc.cpp:440-481
 *                           (callers: EDGraph, fusion_with_occlusion/embedded_deformation_graph.py:153-380,496-609)
 *   ofx_reduce_graph        EDGraph.get_reduced_graph                       embedded_deformation_graph.py:382-477
 *   ofx_graph_downsample    EDGraph.create_graph_pyramid down-sampling      embedded_deformation_graph.py:278-299
 *   ofx_gn_*                DeformNet.optimize Gauss-Newton (JᵀJ, Jᵀr, LU)   model/model.py:222-859 (+ LinearSolverLU :59-86)
 *                           DeformNet.arap (params.mode = OFX_GN_ARAP)       model/model.py:1639-1986
 *                           (LU replaced by warm-started block-Jacobi PCG; ofx_gn_stats: per-step diagnostics)
 */
#ifndef OFX_H
#define OFX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFX_ABI_VERSION 5

typedef void* ofx_stream_t; /* hipStream_t; NULL = legacy default stream */

enum {
  OFX_OK = 0,
  OFX_ERR_ARG = -1,      /* bad argument / shape */
  OFX_ERR_HIP = -2,      /* HIP runtime error */
  OFX_ERR_RANGE = -3,    /* size limit exceeded (e.g. > 65534 nodes) */
  OFX_ERR_STATE = -4,    /* call order violated */
  OFX_ERR_ALLOC = -5
};

const char* ofx_last_error(void);
int ofx_abi_version(void);

/* Voxel volume: dense grid (reference C-order semantics), stored on device as
 * 8x8x8 bricks, brick-major. A shard owns bricks [brick_x0, brick_x1) along x. */
typedef struct ofx_volume_desc {
  int32_t dim[3];       /* Dx, Dy, Dz (TSDFVolume._vol_dim) */
  int32_t brick_x0;     /* first brick column along x owned by this shard */
  int32_t brick_x1;     /* one past the last (full volume: ceil(Dx/8)) */
  int32_t semantics;    /* integrate arithmetic: OFX_SEM_CPU (0) or OFX_SEM_PYCUDA (1) */
  float origin[3];      /* TSDFVolume._vol_origin (f32) */
  float _pad1;
  double voxel_size;    /* TSDFVolume._voxel_size (f64) */
  double trunc_margin;  /* TSDFVolume._trunc_margin (0.04) */
} ofx_volume_desc;

/* Integrate semantics (ofx_volume_desc.semantics). The reference has two integrate paths that compute
 * different numbers:
 *   OFX_SEM_CPU    numba/numpy CPU branch, tsdf.py:442-494: f64 projection, round-half-even pixels,
 *                  update iff depth > 0 and d - z >= -trunc, plain d - z.
 *   OFX_SEM_PYCUDA pycuda kernel, tsdf.py:192-288 (used when fopt.gpu and pycuda import): f32 throughout,
 *                  pixel = (int)roundf(f32(f·x/z + c) + 0.5) (half away from zero), skip iff depth == 0,
 *                  (d - z) scaled by the ray factor sqrt(1 + mx² + my²) of the integer pixel, roundf colours. */
enum { OFX_SEM_CPU = 0, OFX_SEM_PYCUDA = 1 };

typedef struct ofx_camera {
  float fx, fy, cx, cy; /* cam_intr (cast to f32 as tsdf.py:357) */
  int32_t width, height;
} ofx_camera;

/* number of voxel slots (bricks*512) a shard stores */
int ofx_volume_num_slots(const ofx_volume_desc* desc, int64_t* n_slots);

int ofx_volume_reset(const ofx_volume_desc* desc, float* tsdf, float* weight, float* color, ofx_stream_t s);
/* bricked shard -> C-order dense (Dx_shard, Dy, Dz) where Dx_shard = min(8*x1,Dx) - 8*x0 */
int ofx_volume_to_dense(const ofx_volume_desc* desc, const float* bricked, float* dense, ofx_stream_t s);
int ofx_volume_from_dense(const ofx_volume_desc* desc, const float* dense, float* bricked, ofx_stream_t s);

/* rgb (3,H,W) f32 in [0,1] -> packed colour (H,W) f32 (tsdf.py:561-562) */
int ofx_pack_color(const float* rgb, int32_t height, int32_t width, float* packed, ofx_stream_t s);

/* Skinning of the voxel grid.
 * Step 1: list the shard's bricks that can hold a skin-valid voxel (>= K nodes within
 *         4*node_coverage of the brick). brick_list: int32[num_bricks], count: device int32[1].
 * Step 2: per-voxel k-NN for the listed bricks -> anchors uint16[n_list*512*4] (0xFFFF = -1),
 *         weights f32[n_list*512*4]; slot = list position.                                */
int ofx_skin_volume_bricks(const ofx_volume_desc* desc, const float* nodes, int32_t n_nodes,
                           double node_coverage, int32_t k, int32_t* brick_list, int32_t* count,
                           ofx_stream_t s);
int ofx_skin_volume(const ofx_volume_desc* desc, const float* nodes, int32_t n_nodes, double node_coverage,
                    int32_t k, const int32_t* brick_list, int32_t n_list, uint16_t* anchors, float* weights,
                    ofx_stream_t s);
/* Node palette of the bricked skin cache (MI355X-specific, no reference twin): per listed brick the
 * ascending distinct anchors of its skin-valid voxels, pal_ids u16[n_list*OFX_PALETTE], count
 * pal_n i32[n_list] (> OFX_PALETTE: overflow, palette unused), and per voxel the anchors as palette
 * ranks local_anchors u8[n_list*512*4] (0xFF: skin-invalid voxel / unused slot). */
#define OFX_PALETTE 64
int ofx_skin_palette(const uint16_t* anchors, int32_t n_list, int32_t k, int32_t n_nodes, uint16_t* pal_ids,
                     int32_t* pal_n, uint8_t* local_anchors, ofx_stream_t s);
/* In-place update of the skin cache after nodes were appended (ofx_grow_nodes): nodes f32[(n_old + *n_added)*3], n_added a
 * DEVICE int32 (count[1] of ofx_grow_nodes: no host read between the two calls). A voxel's skin can change only if a new
 * node lies within the 4-sigma cut-off of it: a new node farther away that enters its top-K replaces an anchor that was
 * already past the cut-off, and both are written as 0xFFFF with weight 0. So only bricks whose AABB lies within the cull
 * radius of a new node (ofx_skin_volume_bricks' test) need work.
 * ofx_skin_grow_plan: one thread per brick -> the work list, work_bricks / work_slots int32[num_bricks] each: first the
 *   touched bricks of brick_list (ascending brick id) at their existing slots, then the touched unlisted bricks that now
 *   have >= K of all nodes within the cull radius (ascending id: what a full ofx_skin_volume_bricks would add) at slots
 *   n_list, n_list + 1, ...; counts (DEVICE int32[2]) = [re-skinned, appended].
 * ofx_skin_grow_apply: ofx_skin_volume and ofx_skin_palette (the same kernels, a slot indirection) over the first n_work =
 *   re-skinned + appended work entries against all n_nodes nodes; anchors / weights / pal_ids / pal_n / local_anchors are
 *   the cache's arrays enlarged by the caller to n_list + appended slots. The caller appends work_bricks[re-skinned ..
 *   n_work) to its brick list, which is then no longer ascending (ofx_surface_points and ofx_integrate* take any order).
 *   The result equals a full rebuild on the grown node set, slot for brick, bit for bit. */
int ofx_skin_grow_plan(const ofx_volume_desc* desc, const float* nodes, int32_t n_old, const int32_t* n_added,
                       double node_coverage, int32_t k, const int32_t* brick_list, int32_t n_list, int32_t* work_bricks,
                       int32_t* work_slots, int32_t* counts, ofx_stream_t s);
int ofx_skin_grow_apply(const ofx_volume_desc* desc, const float* nodes, int32_t n_nodes, double node_coverage, int32_t k,
                        const int32_t* work_bricks, const int32_t* work_slots, int32_t n_work, uint16_t* anchors,
                        float* weights, uint16_t* pal_ids, int32_t* pal_n, uint8_t* local_anchors, ofx_stream_t s);
/* Skinning of arbitrary points: anchors int32[P*K] (-1 beyond 4σ), weights f32[P*K], valid u8[P] */
int ofx_skin_points(const float* points, int64_t n_points, const float* nodes, int32_t n_nodes,
                    double node_coverage, int32_t k, int32_t* anchors, float* weights, uint8_t* valid,
                    ofx_stream_t s);
/* Expand the bricked skin cache to C-order (V,4) int32 / f32 / valid u8 (testing & API parity). */
int ofx_skin_volume_to_dense(const ofx_volume_desc* desc, const int32_t* brick_list, int32_t n_list,
                             const uint16_t* anchors, const float* weights, int32_t k, int32_t* anchors_out,
                             float* weights_out, uint8_t* valid_out, ofx_stream_t s);

/* Node transforms (node-relative, as Registration.deform_ED uses them):
 * R f32[N*9] row-major, T f32[N*3], g f32[N*3] -> packed f32[N*16], 64-B records interleaved for
 * packed-f32 warps: [R00 R10 R01 R11 | R02 R12 g0 g1 | t0 t1 R20 R21 | R22 g2 t2 0] */
int ofx_pack_nodes(const float* R, const float* T, const float* g, int32_t n_nodes, float* packed,
                   ofx_stream_t s);

/* Fused warp + integrate of one frame into the shard.
 *   warp = 0 : source frame — every voxel, world position, no skin (tsdf.py:395-398); with brick_list
 *              non-NULL (CPU semantics only) just the n_list listed bricks (a hash-bucket shard's own)
 *   warp = 1 : bricks in brick_list, ED-warped positions, skin-valid voxels only (tsdf.py:401,464)
 * color_im / color may be NULL (no colour integration). n_updated (device u32, one entry per launched
 * brick: n_list when a list is given, all shard bricks otherwise) receives per-brick update counts, may
 * be NULL. */
int ofx_integrate(const ofx_volume_desc* desc, const ofx_camera* cam, const float* depth, const float* color_im,
                  int32_t warp, const float* packed_nodes, int32_t n_nodes, int32_t k,
                  const int32_t* brick_list, int32_t n_list, const uint16_t* anchors, const float* weights,
                  double obs_weight, float* tsdf, float* weight, float* color,
                  uint32_t* n_updated, ofx_stream_t s);

/* ofx_integrate (warp = 1) with the skin cache's node palette (ofx_skin_palette): each brick's node
 * records are staged once in LDS. Bit-identical results; bricks with pal_n > OFX_PALETTE fall back
 * to the global anchors. */
int ofx_integrate_palette(const ofx_volume_desc* desc, const ofx_camera* cam, const float* depth,
                          const float* color_im, const float* packed_nodes, int32_t n_nodes, int32_t k,
                          const int32_t* brick_list, int32_t n_list, const uint16_t* anchors, const float* weights,
                          const uint16_t* pal_ids, const int32_t* pal_n, const uint8_t* local_anchors,
                          double obs_weight, float* tsdf, float* weight, float* color, uint32_t* n_updated,
                          ofx_stream_t s);

/* ofx_integrate_palette with a per-frame brick cull in front (CPU semantics, k = 4; otherwise it is
 * ofx_integrate_palette): per 8x8 pixel tile the largest depth (tile_scratch: f32[ceil(W/8)*ceil(H/8)]), then per
 * listed brick a conservative box of its warped voxels (each palette node's rigid image of the brick, scaled by the
 * skin weights' sum range) tested against the camera and those tiles; bricks that provably update no voxel are
 * skipped (active: u8[n_list] receives the flags; n_updated gets 0 for them). Bit-identical results. MI355X-specific:
 * no reference twin (the reference walks every voxel, tsdf.py:442-494). */
int ofx_integrate_palette_cull(const ofx_volume_desc* desc, const ofx_camera* cam, const float* depth,
                               const float* color_im, const float* packed_nodes, int32_t n_nodes, int32_t k,
                               const int32_t* brick_list, int32_t n_list, const uint16_t* anchors, const float* weights,
                               const uint16_t* pal_ids, const int32_t* pal_n, const uint8_t* local_anchors,
                               double obs_weight, float* tsdf, float* weight, float* color, uint32_t* n_updated,
                               float* tile_scratch, uint8_t* active, ofx_stream_t s);

/* Profiling hook (process-wide): returns (and resets) the device time of the warped integrate kernel launches
 * (ofx_integrate warp = 1, ofx_integrate_palette) recorded since the last call, from hipEvents recorded by the
 * library around each launch on its stream (synchronises on them), and their count; `enable` switches
 * recording for the following launches. */
int ofx_integrate_timing(int32_t enable, double* kernel_ms, int64_t* launches);

/* Integrate of explicit (already deformed) points: point p updates the voxel with C-order id voxel_ids[p]
 * (i·Dy·Dz + j·Dz + k) as TSDFVolume.integrate does for pts from WarpField.deform_tsdf (tsdf.py:442-494,
 * warpfield.py:369-380); valid (u8, may be NULL) masks points. Same arithmetic as ofx_integrate (CPU or
 * pycuda semantics). Voxel ids must be distinct; ids outside this shard are ignored. n_updated (one u32,
 * may be NULL) is incremented by the number of updated voxels. */
int ofx_integrate_points(const ofx_volume_desc* desc, const ofx_camera* cam, const float* depth, const float* color_im,
                         const float* points, const int64_t* voxel_ids, const uint8_t* valid, int64_t n_points,
                         double obs_weight, float* tsdf, float* weight, float* color, uint32_t* n_updated,
                         ofx_stream_t s);

/* ---------------- Weighted integrate (new capability; the reference's is the plain running average, tsdf.py:366-376) ----
 * The _w twins of the four integrate entry points: the same arguments plus an ofx_obs_weights, the same kernels
 * instantiated with the weighted update, CPU semantics only. Restated op for op by tests/weighted_ref.py. Per voxel, at
 * the pixel pix it already projects to and with every existing update condition unchanged:
 *   o      = obs_im[pix]; !(o > 0 && o < +inf) (zero, negative, NaN, +inf): the voxel is not updated and not counted
 *   obs    = f64(o) * obs_weight
 *   w_sum  = f32(f64(w_old) + obs)
 *   tsdf'  = f32((f64(f32(w_old * tsdf)) + obs * dist) / f64(w_sum))          (the unweighted flow with obs per voxel)
 *   colour = as unweighted, with ow = f32(obs) and the divisor w_sum
 *   weight' = fminf(w_sum, w_max)                                             (w_max = +inf: no cap)
 * With obs_im == 1 everywhere and w_max = +inf the result equals the unweighted entry point's bit for bit. The brick
 * cull is unchanged (it proves "no voxel updates" from the depth alone; a weight only removes updates).
 * OFX_ERR_ARG: ow or obs_im NULL, obs_im not 4-byte aligned, !(w_max > 0) (a NaN included), OFX_SEM_PYCUDA. */
typedef struct ofx_obs_weights {
  const float* obs_im;  /* device f32[H*W], the depth image's size (e.g. ofx_observation_weights') */
  float w_max;          /* cap on the stored weight, > 0; +inf = off */
  float _pad;
} ofx_obs_weights;
int ofx_integrate_w(const ofx_volume_desc* desc, const ofx_camera* cam, const float* depth, const float* color_im,
                    int32_t warp, const float* packed_nodes, int32_t n_nodes, int32_t k,
                    const int32_t* brick_list, int32_t n_list, const uint16_t* anchors, const float* weights,
                    double obs_weight, float* tsdf, float* weight, float* color,
                    uint32_t* n_updated, const ofx_obs_weights* ow, ofx_stream_t s);
int ofx_integrate_palette_w(const ofx_volume_desc* desc, const ofx_camera* cam, const float* depth,
                            const float* color_im, const float* packed_nodes, int32_t n_nodes, int32_t k,
                            const int32_t* brick_list, int32_t n_list, const uint16_t* anchors, const float* weights,
                            const uint16_t* pal_ids, const int32_t* pal_n, const uint8_t* local_anchors,
                            double obs_weight, float* tsdf, float* weight, float* color, uint32_t* n_updated,
                            const ofx_obs_weights* ow, ofx_stream_t s);
int ofx_integrate_palette_cull_w(const ofx_volume_desc* desc, const ofx_camera* cam, const float* depth,
                                 const float* color_im, const float* packed_nodes, int32_t n_nodes, int32_t k,
                                 const int32_t* brick_list, int32_t n_list, const uint16_t* anchors, const float* weights,
                                 const uint16_t* pal_ids, const int32_t* pal_n, const uint8_t* local_anchors,
                                 double obs_weight, float* tsdf, float* weight, float* color, uint32_t* n_updated,
                                 float* tile_scratch, uint8_t* active, const ofx_obs_weights* ow, ofx_stream_t s);
int ofx_integrate_points_w(const ofx_volume_desc* desc, const ofx_camera* cam, const float* depth, const float* color_im,
                           const float* points, const int64_t* voxel_ids, const uint8_t* valid, int64_t n_points,
                           double obs_weight, float* tsdf, float* weight, float* color, uint32_t* n_updated,
                           const ofx_obs_weights* ow, ofx_stream_t s);

/* TSDF raycast (new capability; the reference has none — parity unpinned, restated by the oracle): per pixel
 * of `cam` (identity pose), march the ray from max(z_near, volume entry) to min(z_far, volume exit) through the
 * trilinear tsdf (unobserved voxels and the outside count as +1), coarse steps of 0.8·trunc while the sample
 * is >= 0.999, one-voxel steps otherwise; the first + -> - sign change, linearly refined, is the surface.
 * depth f32[H*W] (z, 0 = miss); normals f32[H*W*3] (normalised central differences, may be NULL); colors
 * f32[H*W] (packed colour of the nearest voxel, may be NULL; color may be NULL then). Needs the whole volume
 * (brick range [0, nbx)). */
int ofx_raycast(const ofx_volume_desc* desc, const ofx_camera* cam, const float* tsdf, const float* weight,
                const float* color, float z_near, float z_far, float* depth, float* normals, float* colors,
                ofx_stream_t s);

/* ED warp of points: out = Σ w (R(x-g)+g+t) for valid points, x otherwise.
 * normals = 1: WarpField.deform_normals semantics (R only, renormalised). valid may be NULL (all valid). */
int ofx_deform_points(const float* points, int64_t n_points, const int32_t* anchors, const float* weights,
                      const uint8_t* valid, int32_t k, const float* packed_nodes, int32_t n_nodes,
                      int32_t normals, float* out, ofx_stream_t s);

/* WarpField.deform_lbs (origin-form LBS, the use_pytorch=False branch of WarpField.deform):
 * out = Σ_{k: w_k != 0} w_k (R_k x + t_k) for valid points, x otherwise; rotations f32[N*9] row-major,
 * translations f32[N*3] in origin form (t = -R g + g + T). Anchors must be in [0, n_nodes) where w != 0. */
int ofx_deform_points_lbs(const float* points, int64_t n_points, const int32_t* anchors, const float* weights,
                          const uint8_t* valid, int32_t k, const float* rotations, const float* translations,
                          int32_t n_nodes, float* out, ofx_stream_t s);

/* check_visibility: valid u8[P], depth_diff f64[P] */
int ofx_visibility(const float* points, int64_t n_points, const ofx_camera* cam, const float* depth,
                   double trunc_margin, uint8_t* valid, double* depth_diff, ofx_stream_t s);
/* The same check with the projection in f32, as numba runs cam2pix on an f32 point array: get_visible_nodes on
 * the f32 deformed nodes (tsdf.py:614-638 -> 599-612 -> 351-364); depth lookup and depth_diff in f64 */
int ofx_visibility_f32(const float* points, int64_t n_points, const ofx_camera* cam, const float* depth,
                       double trunc_margin, uint8_t* valid, double* depth_diff, ofx_stream_t s);

/* ---------------- Surface extraction ----------------
 * Voxel-index coordinates as skimage returns. ofx_truncated_region / ofx_mesh_count take the whole volume;
 * ofx_mesh_count_range takes a shard whose stored bricks include a halo (see there). */
/* TSDFVolume.compute_truncated_region (tsdf.py:704-745): mask u8 per voxel slot (bricked layout) */
int ofx_truncated_region(const ofx_volume_desc* desc, const float* tsdf, double max_diff, uint8_t* mask,
                         ofx_stream_t s);
/* Marching cubes (measure.marching_cubes at tsdf.py:755,794), two phases on an opaque handle:
 * ofx_mesh_count classifies cells and sizes the output (synchronises the stream), the caller allocates,
 * ofx_mesh_emit writes verts f32[V*3] (voxel coordinates), faces i32[F*3] and optionally normals
 * f32[V*3] (unit, towards increasing tsdf), values f32[V], keys i64[V] (= C-index(edge start)*3 + axis).
 * use_mask = 0: every cell (get_point_cloud); use_mask = 1 with mask = NULL: the volume's truncated region
 * with max_diff (get_mesh, tsdf.py:792); with a mask (bricked u8): that mask. A cell [c, c+1]^3 is
 * processed iff the mask holds at its far corner c+1. */
int ofx_mesh_create(void** handle);
int ofx_mesh_destroy(void* handle);
int ofx_mesh_count(void* handle, const ofx_volume_desc* desc, const float* tsdf, const uint8_t* mask, double max_diff,
                   int32_t use_mask, float level, int64_t* n_verts, int64_t* n_faces, ofx_stream_t s);
int ofx_mesh_emit(void* handle, float* verts, int32_t* faces, float* normals, float* values, int64_t* keys,
                  ofx_stream_t s);
/* Sharded marching cubes: like ofx_mesh_count on a shard desc (bricks [brick_x0, brick_x1), holding the
 * shard's own bricks plus halo bricks copied from its neighbours), processing only the cells whose far corner
 * x lies in [px0, px1) — the shard's own planes. px0 >= 8*brick_x0 + 2 unless brick_x0 = 0, px1 <= 8*brick_x1 - 2
 * unless the shard reaches the volume's end (the truncated-region test and the vertex normals read ±2 planes).
 * The emitted vertices are those the shard's cells use, in global order (keys identify them across shards);
 * the full volume's mesh is the key-merge of the shards' meshes (occlusionfusion_amd.sharding). */
int ofx_mesh_count_range(void* handle, const ofx_volume_desc* desc, const float* tsdf, const uint8_t* mask,
                         double max_diff, int32_t use_mask, float level, int32_t px0, int32_t px1, int64_t* n_verts,
                         int64_t* n_faces, ofx_stream_t s);
/* get_mesh / get_point_cloud epilogue (tsdf.py:757-767,796-807): world = verts*f32(voxel_size) + origin
 * (f32, may be NULL) and colours u8[V*3] = [r,g,b] of the voxel nearest each vertex (may be NULL). */
int ofx_mesh_finish(const ofx_volume_desc* desc, const float* color, const float* verts, int64_t n_verts,
                    float* world, uint8_t* colors, ofx_stream_t s);

/* ---------------- Correspondence front-end ---------------- */
/* backproject_depth: point_image f32[3*H*W] (planar x, y, z); pixels with depth <= 0 are left untouched
 * (the reference zero-fills before the call). depth is f32[H*W] metres (is_u16 = 0) or u16[H*W] scaled by
 * 1/normalizer (is_u16 = 1). Arithmetic as the C++: f32 d*(x-cx)/fx, correctly rounded. */
int ofx_backproject_depth(const void* depth, int32_t is_u16, int32_t height, int32_t width, float fx, float fy, float cx,
                          float cy, float normalizer, float* point_image, ofx_stream_t s);
/* compute_mesh_from_depth on a planar point image f32[3*H*W]; handle owns scratch (also used by
 * ofx_depth_to_pc). count sizes the output (synchronises the stream); emit writes vertices f32[V*3],
 * vertex_pixels i32[V*2] (x, y; may be NULL) and faces i32[F*3], numbered exactly as the sequential C++. */
int ofx_depth_mesh_create(void** handle);
int ofx_depth_mesh_destroy(void* handle);
int ofx_depth_mesh_count(void* handle, const float* point_image, int32_t height, int32_t width,
                         float max_triangle_distance, int64_t* n_verts, int64_t* n_faces, ofx_stream_t s);
int ofx_depth_mesh_emit(void* handle, float* vertices, int32_t* vertex_pixels, int32_t* faces, ofx_stream_t s);
/* depth_2_pc(depth, K) (f64 arithmetic, rounded to f32) of the pixels with depth > 0, row-major:
 * points f32[capacity H*W*3], pix_map i64[H*W] (point index or -1; may be NULL), n_points: DEVICE int32.
 * Asynchronous (no host sync). */
int ofx_depth_to_pc(void* handle, const float* depth, int32_t height, int32_t width, double fx, double fy, double cx,
                    double cy, float* points, int64_t* pix_map, int32_t* n_points, ofx_stream_t s);

/* ---------------- Projective data association (new capability; the reference has none — parity unpinned) ----------------
 * The data term of a depth frame without given matches: each model point is warped with the current node transforms, looked
 * up in the target vertex map at its pixel, gated, and the surviving pairs are compacted for ofx_gn_solve (src / anchors /
 * weights / tgt rows). Per point, the first rejection code that applies:
 *   1  valid[p] == 0 (or an anchor outside [0, n_nodes): it cannot be gathered)
 *   2  warped z <= 0, or non-finite, or the pixel outside the image
 *   3  target depth at the pixel <= 0 (hole)
 *   4  no target normal: the pixel on the image border, a 4-neighbour with z <= 0, a neighbour's z more than edge_max from
 *      the centre's (depth edge), or a zero-length cross product
 *   5  squared distance |q - x'|^2 > dist_max^2
 *   6  normals given and n'.n_q < cos_min
 *   0  accepted
 * Arithmetic (f32, no contraction; every step fixed so that a numpy f32 restatement gives the same bits):
 *   x'  = ofx_deform_points (normals = 0) of the point, bit for bit; n' = its normals = 1 form (the same device code);
 *         a point with valid == 0 keeps its position in `warped`, as there
 *   pixel = the one ofx_visibility_f32 takes for the f32 point x' (the same device function: (x.fx)/z + cx in f32 with a
 *         correctly rounded division, rintf, the range test on the rounded value)
 *   q   = point_image at the pixel (planar f32[3*H*W], the layout ofx_backproject_depth writes)
 *   n_q = normalise((q[v,u+1] - q[v,u-1]) x (q[v+1,u] - q[v-1,u])): a*b - c*d per component, squared length (x^2 + y^2) +
 *         z^2, square root and divisions correctly rounded; flipped if n_q.q > 0 (faces the camera). Dot products are
 *         summed (x + y) + z
 *   tgt = q (OFX_ASSOC_POINT) or x' + n_q*((q - x').n_q) (OFX_ASSOC_PLANE: the foot of x' on q's tangent plane; the solver's
 *         3-D point rows then act as a point-to-plane term for the step and the surface can slide); zeros when rejected
 * Compaction (scan of code == 0, ascending point index): with n accepted, all are emitted if n <= max_matches; otherwise
 * the accepted point of rank r is emitted iff floor((r+1)*max_matches/n) > floor(r*max_matches/n) (64-bit integers) —
 * exactly max_matches rows, evenly and deterministically, where the reference draws an unseeded randperm (model/model.py:
 * 319-334). Emitted rows keep ascending point order: match_idx i32[max_matches] (point indices), src_out f32[.,3] (the
 * un-warped points), tgt_out f32[.,3], anchors_out i32[.,4], weights_out f32[.,4]; count (DEVICE int32[2]) = [accepted,
 * emitted]. Rows past `emitted` are left untouched.
 * Per-point outputs: code u8[P], tgt f32[P,3], warped f32[P,3] (may be NULL). normals f32[P,3] and valid u8[P] may be NULL.
 * anchors i32[P,4] / weights f32[P,4] (K = 4), their compacted twins and packed_nodes (ofx_pack_nodes) must be 16-byte
 * aligned. cam's width / height must equal the image's. Stream-ordered: no allocation and no host sync inside the call;
 * the handle owns the rank and tile scratch, sized at create for max_points (n_points above it is OFX_ERR_ARG).
 * n_points = 0 is legal: count = [0, 0]. */
typedef struct ofx_assoc_params {
  float dist_max;        /* metres */
  float cos_min;
  float edge_max;        /* metres of z between 4-neighbours */
  int32_t mode;          /* OFX_ASSOC_POINT / OFX_ASSOC_PLANE */
  int32_t max_matches;   /* rows of the compacted outputs */
  int32_t _pad;
} ofx_assoc_params;
enum { OFX_ASSOC_POINT = 0, OFX_ASSOC_PLANE = 1 };
int ofx_assoc_create(int64_t max_points, void** handle);
int ofx_assoc_destroy(void* handle);
int ofx_associate(void* handle, const float* points, const float* normals, const int32_t* anchors, const float* weights,
                  const uint8_t* valid, int64_t n_points, const float* packed_nodes, int32_t n_nodes,
                  const ofx_camera* cam, const float* point_image, int32_t height, int32_t width,
                  const ofx_assoc_params* prm, uint8_t* code, float* tgt, float* warped, int32_t* match_idx,
                  float* src_out, float* tgt_out, int32_t* anchors_out, float* weights_out, int32_t* count,
                  ofx_stream_t s);

/* ---------------- Rigid pre-alignment: point-to-plane ICP (new capability; the reference has none — parity unpinned) -------
 * The cheap stage in front of the non-rigid solve: a rigid pose [R|t] (6 unknowns) that brings ALL model points, warped by
 * the current node transforms, onto the depth frame. Inputs and their checks are ofx_associate's. pose is DEVICE f64[12],
 * row-major [R|t], read and written in place. Restated op for op by tests/rigid_ref.py. One iteration, per point (f32, no
 * contraction, every step fixed):
 *   x', n' = ofx_associate's warped point and normalised warped normal (the same device code)
 *   Rf, tf = the f32 roundings of the pose; y_a = ((Rf_a0*x' + Rf_a1*y') + Rf_a2*z') + tf_a; m = Rf n' in the same order,
 *            not renormalised
 *   pixel, q, n_q and the codes 1-6 are ofx_associate's, with y and m in place of x' and n'
 *   accepted: e = q - y, r = (e.n_q summed (x + y) + z), c = y x n_q (a*b - c*d per component), row J = [c, n_q]
 * Reduction in f64: A = sum J^T J (21 upper entries), b = sum J^T r, sum r^2 and the accepted count. Every term is a product
 * of two f32 values (exact in f64); only the sums round. No atomics: cross-lane shuffles per wave, LDS per workgroup, one
 * record per workgroup, the records summed in a fixed order; the grid depends on n_points alone, so two calls and two
 * handles give the same bytes.
 * Solve (f64): A += damping*trace(A)/6*I, 6x6 Cholesky, xi = (omega, v) = A^-1 b, dR = exp(omega) (Rodrigues, series for
 * |omega| < 1e-8), pose <- [dR R | dR t + v].
 * systems (DEVICE f64[iters][32]), row i of iteration i: [0..20] A row-major upper, undamped; [21..26] b; [27] sum r^2;
 * [28] accepted count; [29] status — 0 solved, 1 fewer than min_matches accepted, 2 a non-positive pivot (or a non-finite
 * step), 3 drained: after an iteration that converged (|omega| and |v| both below stop_twist; that iteration's step is
 * applied) or that had a non-zero status; [30] |omega|; [31] |v|. A non-zero status leaves the pose as it is; a drained row
 * is status 3 and zeros. code (may be NULL): u8[P], the codes of the last iteration that ran.
 * Stream-ordered: all iterations are enqueued at once (two launches each), no allocation and no host sync inside; the handle
 * owns the workgroup records, sized at create for max_points (n_points above it is OFX_ERR_ARG). n_points = 0 is legal: status
 * 1 in every row, pose untouched. */
typedef struct ofx_rigid_params {
  float dist_max, cos_min, edge_max;   /* ofx_associate's gates, same meaning */
  int32_t iters;                       /* >= 1 */
  int32_t min_matches;                 /* fewer accepted points: status 1, pose kept (default 6) */
  double damping;                      /* relative: A += damping * trace(A)/6 * I (default 1e-6) */
  double stop_twist;                   /* |omega| and |v| both below it: converged, later iterations drain (0 = never) */
} ofx_rigid_params;
int ofx_rigid_create(int64_t max_points, void** handle);
int ofx_rigid_destroy(void* handle);
int ofx_rigid_icp(void* handle, const float* points, const float* normals, const int32_t* anchors, const float* weights,
                  const uint8_t* valid, int64_t n_points, const float* packed_nodes, int32_t n_nodes,
                  const ofx_camera* cam, const float* point_image, int32_t height, int32_t width,
                  const ofx_rigid_params* prm, double* pose, uint8_t* code, double* systems, ofx_stream_t s);

/* ---------------- Model z-buffer and occlusion gate (new capability; the reference has none — parity unpinned) ----------------
 * The warped model points splatted as oriented discs of world radius rho into a depth and an index image of the live frame,
 * and the occlusion code of every point against that image: what tells the tracker which model points the model itself
 * hides, and what shows the fused model where the camera is. Inputs and their checks are ofx_associate's (K = 4; anchors,
 * weights and packed_nodes 16-byte aligned; normals and valid may be NULL). Restated op for op by tests/splat_ref.py.
 * Per point (f32, no contraction, every step fixed; the first code that applies):
 *   x', n' = ofx_associate's warped point and normalised warped normal (the same device code); a point with valid == 0
 *            keeps its position in `warped` and its normal in `warped_normals`; normals == NULL: n' = (0, 0, -1)
 *   1  valid[p] == 0, or an anchor outside [0, n_nodes)
 *   2  x' non-finite, z' <= 0, or its pixel (u, v) — the one ofx_visibility_f32 / ofx_associate take — off the image
 *   3  back-facing: s = (n'_x*x' + n'_y*y') + n'_z*z', rejected if !(s < 0) (a NaN normal lands here)
 * A live point (none of the above) writes its disc: r_u = clamp(ceilf((fx*rho)/z'), 0, OFX_SPLAT_RMAX), r_v the same with
 * fy (divisions correctly rounded); for every pixel (uu, vv) = (u + du, v + dv), |du| <= r_u, |dv| <= r_v, inside the image:
 *   centre (du = dv = 0): z_p = z', always written — the buffer at a live point's own pixel is never behind the point
 *   others: dx = (f32(uu) - cx)/fx, dy = (f32(vv) - cy)/fy, den = (n'_x*dx + n'_y*dy) + n'_z, z_p = s/den (divisions
 *           correctly rounded: the ray's hit on the point's tangent plane), e = (dx*z_p - x', dy*z_p - y', z_p - z'),
 *           d2 = (e_x^2 + e_y^2) + e_z^2; written only if den < 0 && z_p > 0 && z_p finite && d2 <= rho*rho (a true disc of
 *           radius rho: an ellipse on the image, thin at grazing angles)
 *   the write is a 64-bit unsigned atomic minimum of key = (u64)float_bits(z_p) << 32 | (u32)p on zbuf[vv*W + uu]: z_p is
 *   positive and finite, so its bits order as the float does; exact ties in z go to the lower point index; a minimum does not
 *   depend on arrival order, so two calls and two handles give the same bytes.
 * After all points: depth[pix] = the float of the key's high word (0 where nothing was written), index[pix] = its low word
 * (-1 where nothing was written), and for a live point
 *   4  occluded: (z' - depth[v*W + u]) > occl_margin
 *   0  visible
 * Outputs (each may be NULL): depth f32[H*W], index i32[H*W], code u8[P], warped f32[P,3], warped_normals f32[P,3] (given
 * without normals: OFX_ERR_ARG). H = cam->height, W = cam->width. splat_radius must be finite and >= 0, occl_margin not NaN.
 * Stream-ordered: three launches, no allocation and no host sync inside; the handle owns the u64 z-buffer of max_pixels
 * words and 8 bytes per point of scratch (n_points above max_points, or width*height above max_pixels, is OFX_ERR_ARG).
 * n_points = 0 is legal: depth all 0, index all -1. */
typedef struct ofx_splat_params {
  float   splat_radius;   /* rho, metres: world radius of a point's disc */
  float   occl_margin;    /* metres of z */
  int32_t _pad[2];
} ofx_splat_params;
#define OFX_SPLAT_RMAX 4
int ofx_splat_create(int64_t max_points, int64_t max_pixels, void** handle);
int ofx_splat_destroy(void* handle);
int ofx_splat_points(void* handle, const float* points, const float* normals, const int32_t* anchors, const float* weights,
                     const uint8_t* valid, int64_t n_points, const float* packed_nodes, int32_t n_nodes,
                     const ofx_camera* cam, const ofx_splat_params* prm, float* depth, int32_t* index, uint8_t* code,
                     float* warped, float* warped_normals, ofx_stream_t s);

/* ---------------- Depth-frame preparation: bilateral filter, vertex map, normal map (new capability; the reference has none —
 * parity unpinned) ----------------
 * What the tracker reads a live frame through, in place of ofx_backproject_depth of the raw image: the bilateral-filtered
 * depth, its vertex map and the gate's target normal at every pixel. The integrate keeps reading the raw frame. Restated op
 * for op by tests/prepare_ref.py. Per pixel (f32, no contraction, every step fixed):
 *   D    = the depth in metres: f32 as given (is_u16 = 0) or u16 / normalizer, correctly rounded (is_u16 = 1:
 *          ofx_backproject_depth's expression)
 *   hole: !(D_c > 0) (a NaN included) writes 0 to every output
 *   taps: dv = -radius..radius (outer), du = -radius..radius (inner); the tap N = D[v + dv, u + du] is skipped when it lies
 *          outside the image, when !(N > 0), or when fabsf(diff) > range_cut with diff = N - D_c in f32 — a skipped tap
 *          behaves exactly like a hole, so nothing bleeds across a depth edge
 *   ws   = f32(exp(a_s * f64(du*du + dv*dv))), a_s = -0.5 / (f64(sigma_s) * f64(sigma_s))   (a host table)
 *   wr   = f32(exp(a_r * (f64(diff) * f64(diff)))), a_r = -0.5 / (f64(sigma_r) * f64(sigma_r))
 *   w    = ws * wr; num = num + w * N; den = den + w (f32, from zero, in tap order)
 *   depth_out = num / den, correctly rounded. The centre tap (du = dv = 0) is always taken with w = 1 exactly — what the
 *          formulas give for diff = 0, and held for a +inf centre, whose own diff would be inf - inf — so den >= 1 and radius
 *          0 returns D_c exactly.
 *   point_image = ofx_backproject_depth's vertex of depth_out (the same device function), zeros where !(depth_out > 0);
 *          with radius 0 it is ofx_backproject_depth's output bit for bit wherever the depth is > 0
 *   normal_image = ofx_associate's n_q of point_image at the pixel (the same device function): zeros where its codes 3 or 4
 *          apply (a hole, the image border, a 4-neighbour hole, a neighbour's z more than edge_max from the centre's, a zero
 *          or non-finite cross product), else the normalised cross product, flipped to face the camera
 * depth_out f32[H*W]; point_image f32[3*H*W] planar; normal_image f32[3*H*W] planar, may be NULL. Every output element is
 * written on every call; the input is only read and must not overlap an output. height / width must be >= 1 and equal cam's.
 * Stream-ordered: no handle, no allocation and no host sync inside the call (two launches, one without normal_image). */
typedef struct ofx_prepare_params {
  int32_t radius;      /* 0 .. OFX_PREPARE_RMAX: window (2r+1)^2; 0 = no filtering */
  float sigma_s;       /* pixels, > 0 */
  float sigma_r;       /* metres, > 0 */
  float range_cut;     /* metres, > 0: a neighbour farther than this in depth from the centre is skipped */
  float edge_max;      /* normal map: ofx_associate's edge_max, same meaning */
  float normalizer;    /* u16 input: depth = u16 / normalizer */
} ofx_prepare_params;
#define OFX_PREPARE_RMAX 4
int ofx_prepare_depth(const void* depth, int32_t is_u16, int32_t height, int32_t width, const ofx_camera* cam,
                      const ofx_prepare_params* prm, float* depth_out, float* point_image, float* normal_image,
                      ofx_stream_t s);

/* Observation-weight map of a frame for the weighted integrate (ofx_integrate*_w), from ofx_prepare_depth's vertex map p
 * and normal map n (planar f32[3*H*W] each). Restated op for op by tests/weighted_ref.py. Per pixel (f32, no contraction,
 * the summation order as written, sqrt and divisions correctly rounded):
 *   hole (!(p_z > 0), a NaN included)                 : 0
 *   no normal (n all zero: the gate's codes 3 / 4 — border, a neighbour hole, a depth edge beyond edge_max)
 *                                                     : edge_weight
 *   else c = -((n_x*p_x + n_y*p_y) + n_z*p_z) / sqrt((p_x*p_x + p_y*p_y) + p_z*p_z), clamped to [0, 1], a NaN -> 0
 *        a = 1, c or c*c for cos_power 0 / 1 / 2
 *        s = 1 if z_ref == 0, else min(1, r*r) with r = z_ref / p_z
 *        w = max(w_floor, a*s)
 * obs_im f32[H*W]: every element is written on every call. Stream-ordered: no handle, no allocation, no host sync (one
 * launch). OFX_ERR_ARG: cos_power outside {0, 1, 2}; a negative or non-finite z_ref, w_floor or edge_weight; a NULL or
 * not 4-byte aligned buffer; height or width < 1 or height * width >= 2^31. */
typedef struct ofx_obs_params {
  int32_t cos_power;   /* 0, 1 or 2 */
  float z_ref;         /* metres; 0 = no range term */
  float w_floor;       /* the least weight of a pixel that has a normal */
  float edge_weight;   /* the weight of a pixel with depth but no normal (0: flying pixels are not fused) */
} ofx_obs_params;
int ofx_observation_weights(const float* point_image, const float* normal_image, int32_t height, int32_t width,
                            const ofx_obs_params* prm, float* obs_im, ofx_stream_t s);

/* ---------------- Photometric correspondence search (new capability; the reference has none — parity unpinned) ----------------
 * The stand-in for the reference's flow network, as ofx_associate is for its landmark matcher: each warped model point looks in
 * a (2*radius + 1)^2 window around its own pixel for the live pixel whose colour matches its own best, among the pixels that
 * pass ofx_associate's geometric gates; that pixel's vertex is the point's 3-D target (a tangential constraint for the
 * solver's existing 3-D rows). Takes an ofx_assoc handle and reuses its scratch. Restated op for op by tests/photo_ref.py.
 * Arithmetic: f32, no contraction, every step fixed.
 *   x', n', the pixel (u, v) and the codes 1 and 2 are ofx_associate's (the same device code)
 *   taps: dv = -radius..radius (outer), du = -radius..radius (inner); a tap off the image is skipped (the centre never is).
 *         At a tap, q = point_image, n_q = normal_image, c = color_image at (u + du, v + dv) (planar f32[3*H*W] each;
 *         normal_image as ofx_prepare_depth writes it for point_image: zeros where the gate has no normal)
 *   tap code, the first that applies:
 *     3  !(q_z > 0)
 *     4  n_q is all zero
 *     5  d2 > dist_max^2, d2 = (e_x^2 + e_y^2) + e_z^2, e = q - x'
 *     6  normals given and n'.n_q < cos_min (summed (x + y) + z)
 *     7  !(c2 <= color_max^2), c2 = (dr^2 + dg^2) + db^2, d. = c. - colors[p]. (a NaN colour lands here)
 *     0  eligible, with cost E = c2 + geo_weight*d2 (the product rounded, then the sum)
 *   point: any tap eligible -> code 0, the match is the eligible tap of the smallest E, ties to the first in tap order; tgt =
 *         its q, pixel = its (u + du, v + dv), cost = its E. Otherwise the code is the LARGEST tap code (how far any tap
 *         got; a maximum, so independent of the order) and tgt = 0, pixel = (-1, -1), cost = 0, as for codes 1 and 2.
 * Compaction is ofx_associate's (scan of code == 0, the 64-bit rank-thinning rule, ascending point order, rows past `emitted`
 * left untouched), with pixel_out f32[max_matches,2] = the match pixel — what the solver's target_px / target_py rows take.
 * With radius = 0, color_max = +inf and normal_image = ofx_prepare_depth's (radius 0, the same edge_max) of point_image,
 * code, tgt, warped, count and the compacted arrays equal ofx_associate's in OFX_ASSOC_POINT mode byte for byte.
 * colors f32[P,3] (rgb in [0,1]) is required; normals, valid, warped, pixel, cost and pixel_out may be NULL (pixel_out needs
 * pixel). Null buffers, alignment and the camera / image size are checked as in ofx_associate; also OFX_ERR_ARG: radius
 * outside [0, OFX_PHOTO_RMAX], geo_weight negative or non-finite, a NaN color_max, n_points above the handle's.
 * n_points = 0 is legal: count = [0, 0]. Stream-ordered: no allocation and no host sync inside the call. */
typedef struct ofx_photo_params {
  float dist_max, cos_min;   /* ofx_associate's gates, same meaning, applied to every tap */
  float color_max;           /* a tap is eligible only if its colour distance^2 <= color_max^2 (+inf: off) */
  float geo_weight;          /* 1/m^2: cost = c2 + geo_weight*d2 (>= 0, finite) */
  int32_t radius;            /* 0 .. OFX_PHOTO_RMAX: window (2r+1)^2 around the point's pixel */
  int32_t max_matches;       /* rows of the compacted outputs */
} ofx_photo_params;
#define OFX_PHOTO_RMAX 8
int ofx_photo_associate(void* assoc_handle, const float* points, const float* normals, const float* colors,
                        const int32_t* anchors, const float* weights, const uint8_t* valid, int64_t n_points,
                        const float* packed_nodes, int32_t n_nodes, const ofx_camera* cam, const float* point_image,
                        const float* normal_image, const float* color_image, int32_t height, int32_t width,
                        const ofx_photo_params* prm, uint8_t* code, float* tgt, float* warped, int32_t* pixel,
                        float* cost, int32_t* match_idx, float* src_out, float* tgt_out, int32_t* anchors_out,
                        float* weights_out, float* pixel_out, int32_t* count, ofx_stream_t s);

/* ---------------- Sub-pixel refinement of photometric matches (new capability; the reference has none — parity unpinned) ----------------
 * ofx_photo_associate picks a whole live pixel by the colour of one pixel. This call aligns the (2*half + 1)^2 colour patch
 * around each match's place in a template image (the frame the point's colour came from) with the live frame, starting at the
 * search's pixel: a classical Lucas-Kanade step, translation only, inverse compositional (template gradients, Hessian built
 * once). The refined 3-D target is the vertex map interpolated at the refined pixel; it goes into the solver's existing 3-D
 * rows. No handle, no allocation, no host sync; restated op for op by tests/refine_ref.py.
 * Inputs (device): template_image f32 planar [3*H*W]; template_mask u8[H*W] or NULL (0 = masked; NULL = every pixel valid);
 * color_image f32 planar [3*H*W] (the live frame); point_image f32 planar [3*H*W] (the live vertex map); template_px
 * f32[R,2] (x, y) of each row's point in the template, sub-pixel; init_px f32[R,2] and tgt_in f32[R,3]: the search's
 * pixel_out and tgt_out; count: DEVICE int32[2] as ofx_photo_associate writes it. The rows are 0 .. min(max(count[1], 0),
 * max_rows) - 1, read on the device (the grid is sized from max_rows). Pixel (x, y) has its centre at integer coordinates.
 * Arithmetic: every per-tap term is f32, one rounded operation per step, no contraction; every sum is f64 over exact
 * products of two f32 values; the 2x2 solve is f64; u is kept as f32.
 *   sample S(img, x, y): xf = floorf(x), yf = floorf(y); VALID iff 0 <= xf <= W - 2 and 0 <= yf <= H - 2 (all four neighbours
 *         inside the image; NaN fails); fx = x - xf, fy = y - yf; with p00 = img[yf][xf], p10 = img[yf][xf + 1], p01 =
 *         img[yf + 1][xf], p11 = img[yf + 1][xf + 1]: S = (1 - fy)*((1 - fx)*p00 + fx*p10) + fy*((1 - fx)*p01 + fx*p11).
 *         A template sample is valid only if, besides, none of its four neighbours is masked.
 *   taps: d = (dx, dy), dy = -half..half (outer), dx = -half..half (inner); n_taps = (2*half + 1)^2; three channels each
 *   template, once: T(d) = S(template, tx + (float)dx, ty + (float)dy); g_x(d) = 0.5*(T(d + (1,0)) - T(d - (1,0))), g_y(d) =
 *         0.5*(T(d + (0,1)) - T(d - (0,1))), each neighbour sampled at t + (float)(d +- 1) itself;
 *         Hxx = sum g_x*g_x, Hxy = sum g_x*g_y, Hyy = sum g_y*g_y over taps (outer) and channels (inner);
 *         det = Hxx*Hyy - Hxy*Hxy; lmin = 0.5*((Hxx + Hyy) - sqrt((Hxx - Hyy)^2 + 4*(Hxy*Hxy)))
 *   iteration k = 0 .. iters - 1, from u = init_px: r(d) = S(color_image, u_x + (float)dx, u_y + (float)dy) - T(d);
 *         b_x = sum g_x*r, b_y = sum g_y*r; D_x = (Hyy*b_x - Hxy*b_y)/det, D_y = (Hxx*b_y - Hxy*b_x)/det;
 *         u_x = (float)((double)u_x - D_x), u_y likewise; the row freezes (no further iteration) once |D_x| < eps and
 *         |D_y| < eps, after that update
 *   residual, after the last iteration: r(d) at the final u once more; msr = (sum r*r)/(3*n_taps); ssd = (float)msr
 *   target: tgt = S(point_image plane, u_x, u_y) for the three planes
 * The device sums each lane's taps in order and then the lanes of a row's group in a fixed xor tree, the restatement in tap
 * order: the f64 sums may differ in their last bits, nothing else does. Two calls give the same bytes.
 * status u8[R], the first code that applies (in the order the steps run):
 *   1  init_px or template_px non-finite, or init_px == (-1, -1)
 *   2  a template sample (the +-1 gradient samples included) is off the image or touches a masked pixel
 *   3  !(det > 0), or !(lmin/n_taps >= min_eig)
 *   4  a live sample is off the image in some iteration or in the residual pass
 *   5  max(|u_x - init_x|, |u_y - init_y|) > max_shift (f32) after some iteration's update
 *   6  !(msr <= ssd_max^2) (f64; +inf switches it off; a NaN lands here)
 *   7  one of the four vertex-map neighbours of the final u has !(z > 0), or !(max z - min z <= edge_max)
 *   0  refined
 * Outputs, every row below the count written on every call: px_out f32[R,2] and tgt_out f32[R,3] — the refined u and tgt on
 * status 0, init_px and tgt_in copied otherwise; status; ssd f32[R] — (float)msr for status 0, 6 and 7, 0 otherwise. Rows at
 * or past the count are left untouched; a count of 0 is legal. px_out / tgt_out may not alias init_px / tgt_in.
 * OFX_ERR_ARG, before any device work: null params / count, a null or misaligned buffer (max_rows > 0), half outside
 * [1, OFX_REFINE_HMAX], iters < 1, a negative or non-finite eps, max_shift, min_eig or edge_max, a NaN ssd_max, height or
 * width < 1, max_rows < 0. Stream-ordered. */
typedef struct ofx_refine_params {
  int32_t half;              /* 1 .. OFX_REFINE_HMAX: patch (2*half + 1)^2 */
  int32_t iters;             /* >= 1 */
  float eps;                 /* px: a row freezes once both |D| < eps */
  float max_shift;           /* px: status 5 beyond it (Chebyshev distance from init_px) */
  float min_eig;             /* status 3 below it: smaller eigenvalue of H per tap */
  float ssd_max;             /* status 6 if the mean squared residual exceeds ssd_max^2 (+inf: off) */
  float edge_max;            /* m: ofx_associate's depth-edge gate at the refined pixel's four neighbours */
  int32_t _pad;
} ofx_refine_params;
#define OFX_REFINE_HMAX 4
int ofx_photo_refine(const float* template_image, const uint8_t* template_mask, const float* color_image,
                     const float* point_image, const float* template_px, const float* init_px, const float* tgt_in,
                     const int32_t* count, int32_t max_rows, int32_t height, int32_t width,
                     const ofx_refine_params* prm, float* px_out, float* tgt_out, uint8_t* status, float* ssd,
                     ofx_stream_t s);

/* ---------------- Skinned surface points of the TSDF (new capability; the reference has none — parity unpinned) ----------------
 * The tracking model read off the volume itself: canonical surface points, their outward normals and their anchors and
 * weights, in one pass over the skin cache's listed bricks — what the reference gets per frame from marching cubes plus a
 * k-NN skin of the vertices (tsdf.get_deformed_model / optimizer.update, fusion_tests/lepard_nicp_test.py:471,537). A
 * point's skin is the cached skin of its voxel, the one ofx_integrate* warps that voxel with, so the tracked and the
 * fused model move identically. Restated op for op by tests/surface_ref.py.
 * Inputs: the bricked tsdf and weight of a WHOLE volume (a shard, brick_x0 != 0 || brick_x1 != ceil(Dx/8), is
 * OFX_ERR_ARG; so are volumes of 2^31 voxels or more), and the skin cache as ofx_skin_volume writes it: brick_list
 * int32[n_list], skin_anchors u16[n_list*512*4] (0xFFFF = none), skin_weights f32[n_list*512*4], k == 4 (else OFX_ERR_ARG).
 * Every voxel v = (i, j, k) of every listed brick gets the first code that applies (comparisons written so that NaN fails):
 *   1  brick padding (i >= Dx etc.) or the volume's boundary layer (an index is 0 or dim - 1)
 *   2  !(weight[v] >= w_min)
 *   3  !(phi >= 0 && phi < 1), phi = tsdf[v]: not in front of the surface inside the truncation band
 *   4  one of the six face neighbours has !(weight >= w_min)
 *   5  no face neighbour has phi_n < 0: not next to the zero level
 *   6  degenerate gradient: g_a = phi(+e_a) - phi(-e_a), l2 = (g_x^2 + g_y^2) + g_z^2, len = f32(sqrt(f64(l2))); rejected
 *      if !(l2 > 0), l2 not finite, or phi > len (a Newton step longer than two voxels)
 *   7  skin-invalid: one of its four cached anchors is 0xFFFF (last: only geometric survivors touch the skin cache)
 *   0  accepted
 * Accepted voxel (f32, no contraction, every step fixed):
 *   c_a = f32(f64(origin_a) + voxel_size*f64(i_a))   the voxel position as the integrate kernels form it
 *   n_a = g_a / len, correctly rounded               unit normal towards increasing tsdf (the camera side: the sense of
 *                                                     ofx_mesh_emit's normals, and what ofx_associate expects)
 *   t   = (phi * f32(2*voxel_size)) / len            product rounded to f32, division correctly rounded
 *   p_a = c_a - n_a*t
 *   anchors = the four cached anchors widened to int32, weights = the four cached weights,
 *   voxel = the C-order index (i*Dy + j)*Dz + k
 * Rows: ascending (list slot, in-brick voxel l = (lx*8 + ly)*8 + lz). With n accepted: all are emitted if n <= max_points;
 * otherwise the accepted voxel of rank r is emitted iff floor((r+1)*max_points/n) > floor(r*max_points/n) (64-bit integers;
 * ofx_associate's rule). count (DEVICE int32[2]) = [accepted, emitted]. Outputs, max_points rows each: points f32[.,3],
 * normals f32[.,3], anchors i32[.,4], weights f32[.,4] (both 16-byte aligned), voxel i32[.], valid u8[.]. Emitted rows
 * have valid = 1; rows from `emitted` to max_points are defined too — valid = 0, voxel = -1, zero points / normals /
 * anchors / weights — so the padded arrays go to ofx_associate without a host read-back. code (may be NULL): u8[n_list*512]
 * in (slot, l) order. n_list == 0 is legal: count = [0, 0], every row padding. n_list above the handle's max_bricks is
 * OFX_ERR_ARG. A list entry that is no brick of the volume gives code 1 for its 512 voxels and reads nothing; a brick
 * listed twice is sampled twice (each slot with its own cached skin). Stream-ordered: no allocation and no host sync inside the call; the handle owns the per-brick counts,
 * their scan and the accepted-voxel bit words. Order comes from counts and a scan, never from atomics: two calls give the
 * same bytes. */
int ofx_surface_create(int32_t max_bricks, void** handle);
int ofx_surface_destroy(void* handle);
int ofx_surface_points(void* handle, const ofx_volume_desc* desc, const float* tsdf, const float* weight,
                       const int32_t* brick_list, int32_t n_list, const uint16_t* skin_anchors,
                       const float* skin_weights, int32_t k, float w_min, int32_t max_points, float* points,
                       float* normals, int32_t* anchors, float* weights, int32_t* voxel, uint8_t* valid, uint8_t* code,
                       int32_t* count, ofx_stream_t s);

/* ---------------- Growing the graph from the sampled model (new capability — parity unpinned) ----------------
 * New nodes at model points that no node supports, a spacing apart, with transforms blended from the point's anchors and
 * an edge row each: DynamicFusion's graph update on the rows ofx_surface_points writes. The reference's twin is the host
 * loop of EDGraph.update behind WarpField.find_unreachable_nodes (embedded_deformation_graph.py:496-609, warpfield.py:
 * 462-485), which re-meshes, re-derives geodesic edges and solves ARAP for the transforms. Restated op for op by
 * tests/grow_ref.py. f32, no contraction, every step fixed.
 * Inputs: the padded model rows points f32[M,3], anchors i32[M,4], weights f32[M,4] (both 16-byte aligned), valid u8[M],
 * M = n_points; nodes f32[(n_nodes + max_new),3], R f32[.,9] row-major and T f32[.,3] (node-relative, as ofx_pack_nodes
 * takes them), edges i32[.,k_e] and edge_weights f32[.,k_e] with the same number of rows: rows [0, n_nodes) are read,
 * rows [n_nodes, n_nodes + selected) are written, nothing else is touched.
 * Candidate: row r with valid[r] != 0, its four anchors in [0, n_nodes), a finite point, and dist_min(r) > min_dist
 *   (a NaN fails), dist_min = f32(sqrt(f64(d2))), d2 = min over all nodes of (dx^2 + dy^2) + dz^2 (the ofx_knn_points form;
 *   NaN distances are skipped as fminf does).
 * Selection: the candidates in ascending row order; candidate r is selected iff no EARLIER SELECTED candidate s has
 *   f32(sqrt(f64(d2(r, s)))) < spacing (strict, as the reference's loop), until max_new are selected: the sequential
 *   greedy loop's result. The cap flag is 1 iff a candidate that the loop would have selected next was left out.
 * New node j = n_nodes + rank of the selected row, p its point, a_k / w_k its anchors and weights:
 *   nodes[j] = p
 *   T[j]     = x' - p, x' = ofx_deform_points (normals = 0, k = 4) of p under (R, T, nodes), bit for bit
 *   R[j]     : in f64. q_k = unit quaternion (w, x, y, z) of R[a_k] by Shepperd's form — with tr = (m00 + m11) + m22, the
 *              branch of the largest of (tr, m00, m11, m22), the first of equals: s = 2*sqrt(tr + 1), w = s/4,
 *              x = (m21 - m12)/s, y = (m02 - m20)/s, z = (m10 - m01)/s; or s = 2*sqrt(((1 + m00) - m11) - m22), x = s/4,
 *              w = (m21 - m12)/s, y = (m01 + m10)/s, z = (m02 + m20)/s; and cyclically — divided by its norm
 *              sqrt(((w^2 + x^2) + y^2) + z^2) (identity if that is not positive and finite); q_k negated if its dot
 *              product with q_0, ((w w' + x x') + y y') + z z', is < 0; acc = w_0*q_0, then acc += w_k*q_k for k = 1..3;
 *              q = acc / norm(acc) (identity if not positive and finite);
 *              R = [1 - 2(yy + zz), 2(xy - zw), 2(xz + yw); 2(xy + zw), 1 - 2(xx + zz), 2(yz - xw); 2(xz - yw), 2(yz + xw),
 *              1 - 2(xx + yy)], each entry rounded to f32. No libm call but sqrt.
 *   edges[j] : the k_e nearest OTHER nodes among all n_nodes + selected, ascending by (d2, id), -1 past the node count;
 *   edge_weights[j] : w_i = f32(exp(f64(-(d*d) / (2c^2)))) with d = f32(sqrt(f64(d2))), the quotient correctly rounded and
 *              2c^2 = (2*node_coverage)*node_coverage in f32; divided by their f32 sum in order (by their number if the
 *              sum is 0), 0 where the edge is -1 (ofx_edges_geodesic's weights with Euclidean distances). Rows of old
 *              nodes are not rewritten: the ARAP block of an edge (i, j) couples both nodes in J^T J anyway.
 * count (DEVICE int32[3]) = [candidates, selected, cap flag]. n_points == 0 or max_new == 0 is legal: count = [0, 0, 0],
 * nothing else happens (the other buffers are not looked at then, and may be NULL). Refused: null buffers, k_e outside [1, 8], n_points or max_new above the handle's, n_nodes < 1,
 * spacing or node_coverage not positive and finite, NaN min_dist (OFX_ERR_ARG); n_nodes + max_new > 65534, and at create
 * max_points > 65536 or max_new > 4096 (OFX_ERR_RANGE: the selected positions live in LDS). Stream-ordered: no
 * allocation and no host sync inside the call; the handle owns the flags, ranks and row lists. Order comes from a scan and
 * a single-workgroup loop, never from atomics: two calls give the same bytes. */
int ofx_grow_create(int32_t max_points, int32_t max_new, void** handle);
int ofx_grow_destroy(void* handle);
int ofx_grow_nodes(void* handle, const float* points, const int32_t* anchors, const float* weights,
                   const uint8_t* valid, int32_t n_points, float* nodes, int32_t n_nodes, float* R, float* T,
                   int32_t* edges, float* edge_weights, int32_t k_e, float node_coverage, float min_dist, float spacing,
                   int32_t max_new, int32_t* count, ofx_stream_t s);

/* ---------------- Standalone skinning / anchors ---------------- */
/* csrc twins, exact (Eigen summation order, list tie order, f32 weights): outputs (H, W, 4) images,
 * anchors i32 (-1 = none) and weights f32, fully (re)initialised by the call. point_image planar f32[3*H*W]. */
int ofx_pixel_anchors_euclidean(const float* nodes, int32_t n_nodes, const float* point_image, int32_t height,
                                int32_t width, float node_coverage, int32_t* pixel_anchors, float* pixel_weights,
                                ofx_stream_t s);
/* node_to_vertex_distance f32[N*V] (row per node, < 0 = unreachable), valid_nodes_mask i32[N],
 * vertex_pixels i32[V*2] (x, y). */
int ofx_pixel_anchors_geodesic(const float* node_to_vertex_distance, const int32_t* valid_nodes_mask, int32_t n_nodes,
                               int64_t n_vertices, const int32_t* vertex_pixels, int32_t width, int32_t height,
                               float node_coverage, int32_t* pixel_anchors, float* pixel_weights, ofx_stream_t s);
/* anchors[i] = id_map[anchors[i]] for anchors[i] != -1 (in place). An anchor with no mapping (outside
 * [0, n_map) or mapped to -1; std::map::at would throw) is left as is and counted into *n_missing (DEVICE
 * int32, accumulated: zero it first). */
int ofx_remap_anchors(int32_t* anchors, int64_t n, const int32_t* id_map, int32_t n_map, int32_t* n_missing,
                      ofx_stream_t s);
/* k nearest nodes (k <= 8) of each point: idx i32[P*k] ascending by (squared distance, node id), -1 past
 * n_nodes; sq_dist f32[P*k] = (dx²+dy²)+dz² in f32. */
int ofx_knn_points(const float* points, int64_t n_points, const float* nodes, int32_t n_nodes, int32_t k, int32_t* idx,
                   float* sq_dist, ofx_stream_t s);

/* ---------------- ED-graph construction ----------------
 * Bit-exact with the compiled reference C++ (tests/test_gpu_graph.py). Graph building runs at init and on
 * graph updates; these entry points synchronise the stream where an output size or a convergence test is
 * needed. A handle keeps the mesh's vertex adjacency; it references (does not copy) vertices f32[V*3] and
 * faces i32[F*3], which must stay alive until ofx_graph_destroy. */
int ofx_graph_create(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, void** handle,
                     ofx_stream_t s);
int ofx_graph_destroy(void* handle);
int ofx_graph_adjacency(void* handle, int32_t* rowptr, int32_t* col, int64_t* n_col, ofx_stream_t s);
/* non_eroded u8[V] */
int ofx_erode_mesh(void* handle, int32_t n_iterations, int32_t min_neighbors, uint8_t* non_eroded, ofx_stream_t s);
/* node_positions f32[V*3] / node_indices i32[V] capacity; *n_nodes written (host); *n_rounds: batches of the
 * single-workgroup greedy form (meshes up to ~1.29M vertices), else launches of the parallel round form
 * (OFX_SN_ROUNDS=1 forces it; OFX_SN_STAMPS=1 prints the greedy form's phase times to stderr) */
int ofx_sample_nodes(void* handle, const uint8_t* non_eroded, float node_coverage, int32_t use_only_non_eroded,
                     float* node_positions, int32_t* node_indices, int64_t* n_nodes, int64_t* n_rounds,
                     ofx_stream_t s);
/* graph_edges i32[N*K] (-1 padded), weights / distances f32[N*K] (0 padded), node_to_vertex_distances f32[N*V]
 * (-1 where unvisited; may be NULL). valid_vertices u8[V] may be NULL (all valid). K <= 16. Reaching an
 * invalid vertex with allow_only_valid_vertices (the reference calls exit(0)) returns OFX_ERR_STATE. */
int ofx_edges_geodesic(void* handle, const uint8_t* valid_vertices, const int32_t* node_indices, int32_t n_nodes,
                       int32_t n_max_neighbors, float node_coverage, int32_t allow_only_valid_vertices,
                       int32_t enforce_total_num_neighbors, int32_t* graph_edges, float* graph_edges_weights,
                       float* graph_edges_distances, float* node_to_vertex_distances, ofx_stream_t s);
/* nodes the last ofx_edges_geodesic on this handle settled with the sequential heap kernel (distance ties
 * the parallel relaxation cannot order, or a neighbourhood larger than its LDS table); the rest were settled
 * by the parallel form. OFX_GEO_SEQ=1 in the environment forces the sequential kernel for every node,
 * OFX_GEO_BIG=1 the 16384-slot parallel form (tests / tuning; results are identical either way). */
int ofx_graph_geodesic_sequential(void* handle, int64_t* n_nodes);
/* one level of EDGraph.create_graph_pyramid's down-sampling (embedded_deformation_graph.py:278-299):
 * down_idx i32[n] (first *n_down valid: kept node indices, ascending), up_idx i32[n] (per node: argmin index
 * INTO the kept list, as the reference). At most 8192 kept nodes (else OFX_ERR_RANGE). Synchronises. */
int ofx_graph_downsample(const float* node_positions, int32_t n_nodes, double node_coverage, int32_t* down_idx,
                         int32_t* up_idx, int32_t* n_down, ofx_stream_t s);
int ofx_edges_euclidean(const float* node_positions, int32_t n_nodes, int32_t n_max_neighbors, int32_t* graph_edges,
                        ofx_stream_t s);
/* valid_in / valid_out u8[N] (may alias) */
int ofx_node_edge_cleanup(const int32_t* graph_edges, int32_t n_nodes, int32_t max_neighbors, const uint8_t* valid_in,
                          uint8_t* valid_out, ofx_stream_t s);
/* clusters i32[N]; cluster_sizes i32[N] capacity (may be NULL); *n_clusters (host) */
int ofx_compute_clusters(const int32_t* graph_edges, int32_t n_nodes, int32_t max_neighbors, int32_t* clusters,
                         int32_t* cluster_sizes, int32_t* n_clusters, ofx_stream_t s);

/* get_reduced_graph: keep the nodes with valid_nodes_mask (u8[N]) in order; edges to removed nodes are
 * dropped (compacted left, ids remapped) and the weights renormalised by f32(f64(np.sum) + 1e-6) as numpy 1.26
 * evaluates it; if no node is removed the rows are copied unchanged. clusters / clusters_out may be NULL.
 * Outputs sized for N rows; *n_kept (host). */
int ofx_reduce_graph(const uint8_t* valid_nodes_mask, int32_t n_nodes, int32_t max_neighbors, const float* nodes,
                     const int32_t* edges, const float* edges_weights, const float* edges_distances,
                     const int32_t* clusters, float* nodes_out, int32_t* edges_out, float* weights_out,
                     float* distances_out, int32_t* clusters_out, int32_t* n_kept, ofx_stream_t s);

/* ---------------- Dense SPD solve (the exact Gauss-Newton step of small graphs) ----------------
 * A x = b in f64 by a right-looking blocked Cholesky (LinearSolverLU's role, model/model.py:59-86). A is n x n, row-major
 * with stride lda >= n; only its lower triangle is read, and it is overwritten by the factor L (A = L Lᵀ; the strict upper
 * triangle is left as given). b (n) is overwritten by x. status (device int32[2]) = [1 if a pivot was <= 0 or not finite
 * (A is not positive definite), index of the first such pivot]; x is all zeros then. Stream-ordered: no host sync, no
 * allocation. One launch per 64-column panel step (panels + 2 in all) and one per panel of the backward solve; the only
 * dependencies between workgroups are the launch boundaries, every sum runs in a fixed order (two runs are bit-identical). 1 <= n <= 3072, else
 * OFX_ERR_RANGE. */
int ofx_spd_solve(double* A, int32_t n, int32_t lda, double* b, int32_t* status, ofx_stream_t s);

/* ---------------- Gauss-Newton (DeformNet.optimize) ---------------- */
typedef struct ofx_gn_params {
  int32_t num_iter;          /* 10 (model.py:91) */
  int32_t use_edge_weighting;/* 0 (custom_settings.py:41) */
  int32_t pcg_max_iter;      /* inner PCG cap */
  int32_t pcg_warm;          /* 1: start each GN step's PCG from the Galerkin projection of b onto the
                                last 4 GN-step solutions (A-norm optimal in that span); 0: x0 = 0 */
  double lambda_flow;        /* 0   (model.py:96) — squared weights, sqrt taken inside (model.py:374-377) */
  double lambda_depth;       /* 1   (model.py:101) */
  double lambda_arap;        /* 0.5 (model.py:105) */
  double lambda_motion;      /* 1   (model.py:108) */
  double lm_factor;          /* 1e-7 (model.py:111) */
  double stop_loss_diff;     /* 1   (model.py:114) */
  double pcg_tol;            /* relative residual target of the inner solve */
  int32_t mode;              /* OFX_GN_OPTIMIZE (0): DeformNet.optimize; OFX_GN_ARAP (1): DeformNet.arap */
  int32_t precond_every;     /* the cluster preconditioner is rebuilt on GN steps gn_iter % precond_every == 0
                                (0 or 1: every step) and reused by the warm-started steps in between; it only
                                shapes convergence, the stop test is unchanged */
  double pcg_err_tol;        /* error-based stop (> 0; ABI 5: one Euclidean estimate for every preconditioner): the
                                inner solve also runs until the estimated Euclidean norm of its solution error
                                sqrt(gamma * mu / theta) <= pcg_err_tol (default 2e-6, a fifth of the 1e-5 bar), with
                                gamma = r^T M^-1 r (||e||_A^2 <= gamma / theta), mu = ||p||^2 / p^T A p of the last
                                search direction (||e||_2^2 ~ ||e||_A^2 mu, Hestenes-Stiefel), theta = the smallest
                                Ritz value of the preconditioned operator's Lanczos tridiagonal (from below, within a
                                factor 2^(1/4) down to 2^-10, sqrt 2 below), or, on GN steps after the first, the
                                previous step's final theta when that is smaller; 0: the relative residual alone. Both
                                stop at a relative residual of 1e-12 */
  double precond_rot_tol;    /* adaptive preconditioner refresh (> 0): a GN step also rebuilds the cluster inverse
                                when some node has rotated by more than this (radians, summed |omega| of the
                                steps since the last rebuild); real data with large rotations (the moose demo)
                                needs it, the synthetic bench never reaches it. 0: precond_every alone */
  int32_t precond;           /* PCG preconditioner: OFX_PRECOND_SCHWARZ (1): overlapping additive Schwarz over the
                                8-node clusters extended by up to 16 coupled ring nodes (two launches per PCG
                                iteration, ~3.4x fewer iterations on the bench graph); OFX_PRECOND_CLUSTER (0): the
                                clusters' block Jacobi (one launch per iteration); OFX_PRECOND_AUTO (2, default of the
                                Python API): Schwarz for graphs of >= 1536 nodes, where the cluster blocks' iteration
                                count has grown past what two launches per iteration and the per-solve subdomain
                                inversion cost (config 2's 1020 nodes: 464.7 vs 419.2 frames/s; config 3's 1998:
                                292 vs 378; config 4's 4016: 106.5 vs 159.9). The Schwarz form needs the wave-list PCG
                                (every 8-row wave <= 128 blocks, rows <= 20 blocks) and falls back to the cluster
                                blocks otherwise. OFX_PRECOND_DIRECT (3) selects the linear solver itself, not a
                                preconditioner: every GN step is solved exactly by a dense f64 Cholesky (ofx_spd_solve's
                                launches) — no PCG, no stop rule, no host synchronisation inside the solve; pcg_* and
                                precond_* are ignored, pcg_iterations and pcg_capped_steps read 0. It serves
                                OFX_GN_OPTIMIZE on graphs of at most 512 nodes (3072 unknowns, a 75 MB dense buffer
                                allocated at first use and kept on the handle); a larger graph is OFX_ERR_RANGE at
                                setup, never a fallback to an estimated solve. OFX_GN_ARAP keeps the cluster PCG
                                (ofx_gn_solver_info tells which ran). OFX_PRECOND_AUTO never picks it */
  int32_t _pad1;
} ofx_gn_params;
enum { OFX_PRECOND_CLUSTER = 0, OFX_PRECOND_SCHWARZ = 1, OFX_PRECOND_AUTO = 2, OFX_PRECOND_DIRECT = 3 };

/* OFX_GN_ARAP restates DeformNet.arap (model/model.py:1639-1986), the graph-update solve for nodes
 * that are invisible or new: no match rows (n_matches = 0); node_conf = valid-node mask (1/0) and
 * target_node_pos = the valid nodes' targets; per valid node three "flow" rows
 * r = sqrt(lambda_flow)·(g + t - target) whose Jacobian on t is r itself (model.py:1772-1784, as
 * written); ARAP rows as in optimize; only nodes with node_conf == 0 are updated (:1940-1943). With
 * lambda_flow = 0 (model.py:98) the system's exact null space (a common translation of each
 * connected graph component) is projected out of every step, as the dense LU solution has none. */
enum { OFX_GN_OPTIMIZE = 0, OFX_GN_ARAP = 1 };

typedef struct ofx_gn_problem {
  int32_t n_nodes, n_matches, n_neighbors, _pad;
  const float* nodes;           /* (N,3) */
  const int32_t* edges;         /* (N,n_neighbors), -1 padded */
  const float* edge_weights;    /* (N,n_neighbors) or NULL */
  const float* target_node_pos; /* (N,3) motion-complete targets */
  const float* node_conf;       /* (N) */
  const float* src;             /* (M,3) */
  const int32_t* anchors;       /* (M,4) all >= 0 */
  const float* weights;         /* (M,4) */
  const float* tgt;             /* (M,3) */
  const float* target_px;       /* (M) or NULL (only used if lambda_flow != 0) */
  const float* target_py;
  const float* prev_rot;        /* (N,9) or NULL -> identity */
  const float* prev_trans;      /* (N,3) or NULL -> zero */
  float fx, fy, cx, cy;
} ofx_gn_problem;

/* status (device int32[5]): [valid_solve, gn_iterations_accepted, pcg_iterations_total, ill_posed,
 * pcg_capped_steps] — the last: GN steps whose PCG stopped at pcg_max_iter without meeting its stop rule (the step
 * was taken with that iterate)
 * loss_log (device f64[num_iter*4]): per accepted iteration [total, data, arap, motion] */
typedef struct ofx_gn_result {
  float* rot;        /* (N,9) */
  float* trans;      /* (N,3) */
  int32_t* status;
  double* loss_log;
} ofx_gn_result;

/* max_nodes <= 8192 (the JᵀJ slot map is dense over the padded rows) */
int ofx_gn_create(int32_t max_nodes, int32_t max_matches, void** handle);
/* Profiling hook: returns (and resets) the device time of the PCG iteration loops recorded since the
 * last call (hipEvents on the solve stream; synchronises on them), the number of PCG launches (k_pcg_iter
 * launches) and of timed solves; `enable` switches recording for the
 * following steps. Under OFX_PRECOND_DIRECT: the device time and the launches of the dense solve (scatter, Cholesky
 * panel steps, backward solve, solution write-back) in their place. */
int ofx_gn_timing(void* handle, int32_t enable, double* pcg_ms, int64_t* iter_launches, int64_t* n_solves);
/* info (host int64[5]) = [n_nodes, n_matches, JᵀJ block count (nnzb), residual terms, rows] of the last
 * setup; rows = nodes in preconditioner-cluster order padded to whole clusters of 8 (<= 2·n_nodes + 8) */
int ofx_gn_info(void* handle, int64_t* info);
/* The preconditioner of the last setup (bench / tools; synchronises the device): info[8] = [Schwarz active, clusters,
 * apply segments (inverse rows of all output clusters), source subdomains, gathered rows, subdomain rows, entries per
 * segment row, kernel launches per PCG iteration (ABI 5: 1 = the one-launch Schwarz iteration k_as_iter, 2 = k_pcg_iter
 * + k_as_apply; 1 for the cluster blocks)]. */
int ofx_gn_precond_info(void* handle, int64_t* info);
/* The linear solver of the last setup: info[4] = [direct active (OFX_PRECOND_DIRECT serving this problem), unknowns
 * n = 6·n_nodes, panel width of the dense Cholesky (0 under the PCG), kernel launches per GN step of the direct path
 * (scatter, the Cholesky panel steps, the backward solve, solution write-back and the GN update; 0 under the PCG)].
 * No synchronisation. */
int ofx_gn_solver_info(void* handle, int64_t* info);
/* Waves per PCG cluster workgroup of k_pcg_iter for the last setup (before any: for a small problem): 2 up to
 * 384 clusters (default) or 1 (environment OFX_PCG_W1 set to anything but "" / "0" at create; tuning and A/B
 * only); larger problems always run one wave per cluster. */
int ofx_gn_pcg_waves(void* handle, int32_t* waves);
/* 1 if the last ofx_gn_step's GN update was taken by its converging PCG launch (its stop flag, ofx_gn_stopped, is
 * then already visible to the host when ofx_gn_step returns); 0 if k_step runs as its own launch (the PCG hit
 * pcg_max_iter, or the arap null-space projection runs first): the flag is written asynchronously. */
int ofx_gn_step_fused(void* handle, int32_t* fused);
/* The solve's stop flag as the host sees it (host-mapped, no synchronisation): 1 once a GN step's loss rule
 * (model.py:726-732) or an ill-posed solve stopped it. The device writes it asynchronously: a stepped multi-rank
 * loop reads it only after synchronising the stream behind ofx_gn_step(i), so that every rank leaves after the
 * same step (GaussNewtonSolver.optimize_distributed). */
int ofx_gn_stopped(void* handle, int32_t* stopped);
/* Per-GN-step statistics of the last solve: out (host f64[3*cap]) = [PCG iterations, |b|², loss] per
 * step (zeros for steps that did not run); synchronous D2H copy, at most 64 steps. */
int ofx_gn_stats(void* handle, double* out, int32_t cap);
/* Row order of the last setup: perm (host int32[cap]) = node of each PCG row, -1 for padding rows
 * (the order of rhs and of the solver's per-node state); cap must be >= rows (ofx_gn_info()[4]). */
int ofx_gn_row_order(void* handle, int32_t* perm, int32_t cap);
int ofx_gn_destroy(void* handle);
/* Upload + build the block-sparse JᵀJ pattern (co-anchored node pairs, edges, diagonal).
 * Copies nodes/edges to the host (one stream sync) to order the rows by graph clusters when the
 * graph changed, and synchronises once more to size the pattern; *nnz_blocks receives the block count. */
int ofx_gn_setup(void* handle, const ofx_gn_problem* prob, const ofx_gn_params* params, int64_t* nnz_blocks,
                 ofx_stream_t s);
/* Assemble A (f64[nnz_blocks*36]) and rhs (f64[6·rows+4]: b = -Jᵀr then [loss² total,data,arap,motion])
 * from matches [m0,m1); regularizers (ARAP, motion) and the LM damping λ_k·I of the diagonal blocks
 * (model.py:418-419,641-662) added iff add_reg. Zeroes both first.
 * In a multi-GPU solve every rank calls this on its match shard, the caller all-reduces
 * (sum) A and rhs, then every rank calls ofx_gn_step with identical buffers. */
int ofx_gn_linearize(void* handle, int32_t gn_iter, int32_t m0, int32_t m1, int32_t add_reg, double* A,
                     double* rhs, ofx_stream_t s);
/* Cluster block-Jacobi PCG solve of A x = b, early-stop bookkeeping, R <- exp(x_rot) R, t += x_t. */
int ofx_gn_step(void* handle, int32_t gn_iter, double* A, double* rhs, ofx_stream_t s);
int ofx_gn_finish(void* handle, const ofx_gn_result* res, ofx_stream_t s);
/* setup + num_iter x (linearize + step) + finish, single device */
int ofx_gn_solve(void* handle, const ofx_gn_problem* prob, const ofx_gn_params* params,
                 const ofx_gn_result* res, ofx_stream_t s);
/* Prefetch the setup of the NEXT problem on this handle (software pipelining across frames; no reference
 * twin — the reference sets up every solve inline, model.py:222-415). Returns at once: the setup (upload,
 * JᵀJ pattern, contribution lists, with its one host sync) runs on a host thread and on the handle's own
 * stream, ordered after everything enqueued on `s` so far, concurrently with the caller's other work (the
 * current frame's solve on another handle). The following ofx_gn_solve on this handle with the same problem
 * (same buffers and sizes, same params; prev_rot / prev_trans may differ: they are read by the solve)
 * skips its setup, waits for the prefetched one on its own stream and loads the pose. A different problem,
 * or a prefetch that failed, falls back to the inline setup. The problem's buffers must stay allocated and
 * unchanged until that solve. */
int ofx_gn_prepare(void* handle, const ofx_gn_problem* prob, const ofx_gn_params* params, ofx_stream_t s);
/* ofx_gn_prepare, started later: the prefetch's host thread waits until the next ofx_gn_solve on `trigger`
 * (another handle) has queued the first kernels of GN step `gn_step`, or returns, or ofx_gn_prepare_wait /
 * ofx_gn_solve / ofx_gn_destroy on this handle needs it. The setup's kernels then overlap that solve's last steps
 * instead of following them. The ordering on `s` is taken now, as for ofx_gn_prepare. */
int ofx_gn_prepare_after(void* handle, const ofx_gn_problem* prob, const ofx_gn_params* params, ofx_stream_t s,
                         void* trigger, int32_t gn_step);
/* Wait (host) until a prefetch on this handle has been enqueued, and order stream `s` after it: a
 * synchronisation of `s` afterwards covers the prefetched setup. */
int ofx_gn_prepare_wait(void* handle, ofx_stream_t s);
/* Make `handle` use `other`'s per-GN-step PCG iteration history (it sizes the first chunk of iteration
 * launches; results do not depend on it): the solver slots of one frame loop then predict from the previous
 * frame whichever slot solved it. */
int ofx_gn_share_history(void* handle, void* other);
/* Solves on this handle that used a prefetched setup / discarded one (a different problem or a failure). */
int ofx_gn_prefetch_stats(void* handle, int64_t* used, int64_t* missed);
/* Host work to run once inside the next solve on this handle, while its host loop waits for the first GN step's PCG
 * chunk (the host is otherwise idle there): fn(arg) is called on the solving thread, then forgotten; NULL fn clears a
 * pending one. A frame loop uses it to enqueue the previous frame's integrate (on a stream of its own) without holding
 * back the next solve's first launches. (Round 6; no ABI struct changes.) */
int ofx_gn_set_idle_hook(void* handle, void (*fn)(void*), void* arg);

/* Per-match weights and a robust kernel (M-estimator, IRLS) on the data rows of OFX_GN_OPTIMIZE: match m's residual
 * triple and Jacobian rows are multiplied by s_m = match_weights[m] · s_rob(e_m), with e_m = |p_m - tgt_m| the match's
 * geometric distance in metres at the current linearisation (independent of the lambdas and of the flow rows):
 *   OFX_ROBUST_NONE   s_rob = 1
 *   OFX_ROBUST_HUBER  s_rob = 1 for e <= scale, sqrt(scale / e) beyond
 *   OFX_ROBUST_TUKEY  s_rob = 1 - (e / scale)² for e < scale, 0 beyond (the square root of the biweight)
 * s is recomputed at every GN step. The ARAP and motion rows, the OFX_GN_ARAP mode and matches outside the [m0, m1) of
 * ofx_gn_linearize are untouched. (ABI 5: a new struct and a new entry point, no existing struct changes.) */
enum { OFX_ROBUST_NONE = 0, OFX_ROBUST_HUBER = 1, OFX_ROBUST_TUKEY = 2 };
typedef struct ofx_gn_robust {
  const float* match_weights;  /* (M) device, or NULL = all 1. Multiplies match m's residual and Jacobian rows, as
                                  correspondence_weights does in DeformNet.forward (model/model.py:1338,1374-1378;
                                  objective weight = its square). The sign is immaterial; a non-finite weight makes
                                  the solve invalid */
  int32_t kernel;              /* OFX_ROBUST_NONE 0 / OFX_ROBUST_HUBER 1 / OFX_ROBUST_TUKEY 2 */
  int32_t _pad;
  double scale;                /* metres, > 0 when kernel != NONE: Huber delta / Tukey c */
} ofx_gn_robust;
/* Sticky on the handle until replaced or cleared (r = NULL, or no weights and OFX_ROBUST_NONE: off, the solver as it
 * is without this call). The next ofx_gn_setup / ofx_gn_solve / ofx_gn_prepare[_after] on the handle copies
 * match_weights into an array of the handle's (stream-ordered, with the problem's upload); the pointer is not read
 * after that setup. A prefetched setup is used by ofx_gn_solve only if it was prepared under the handle's current
 * setting (same pointer, kernel and scale); otherwise it counts as missed and the setup runs inline. An unknown kernel,
 * or a kernel with a scale that is not finite and > 0, is refused (OFX_ERR_ARG); device values are not checked. */
int ofx_gn_set_robust(void* handle, const ofx_gn_robust* r);

/* ---- motion completion network (OcclusionFusion's MotionCompleteNet, motion_model.py:7-98; inference only) ----
 * The network that fills the solver's motion term (target_node_pos, node_conf): a 2-layer LSTM over each node's motion
 * history, then a graph transformer over the 4-level pyramid of the ED graph, in f32; and the runner's pre- and
 * post-processing (fusion_with_occlusion/run_motion_model.py:45-196) in f64. The LSTM and the Linear / LayerNorm layers
 * are pinned to torch's own modules; the graph layers (TransformerConv, DeepGCNLayer 'res+') are restated from their
 * definition and are unpinned against the reference. Yardstick: tests/motion_ref.py, in f64.
 * (ABI 5: new entry points and a new struct, no existing struct changes.)
 *
 * ofx_motion_create: weights is a HOST pointer to the packed f32 blob that occlusionfusion_amd.motion.pack_weights
 * builds (word 0 the layout tag, word 1 the length, both as uint32 bit patterns; then the tensors, transposed for the
 * kernels). A wrong length or tag is OFX_ERR_ARG; max_nodes above 16384 is OFX_ERR_RANGE; max_hist in [1, 16].
 * Synchronous (one host-to-device copy). */
typedef struct ofx_motion_graph {
  const int32_t* nn_index[4];  /* device, (n[l], k[l]) row-major: the neighbours of level l's nodes, -1 = none. Edge
                                  (s, d): s the row, d the listed neighbour (run_motion_model.py:134-148); messages go
                                  s -> d. An entry outside [0, n[l]) counts as -1; duplicates count twice */
  int32_t n[4];                /* nodes per level, 1 .. max_nodes */
  int32_t k[4];                /* list length per level, 1 .. 16 */
  const int32_t* down[3];      /* device, down[l] (n[l+1]): the level-l node each level-(l+1) node is */
  const int32_t* up[3];        /* device, up[l] (n[l]): the level-(l+1) node each level-l node reads coming back up.
                                  Map entries are clamped into their range */
} ofx_motion_graph;
int ofx_motion_create(const float* weights, int64_t n_floats, int32_t max_nodes, int32_t max_hist, void** handle);
int ofx_motion_destroy(void* handle);
/* Copies the lists and maps (stream-ordered; the caller's arrays are free after the call's work has run) and builds on
 * the device the incoming-edge CSR of every level, ordered by (target, source row, slot) — the edge-list order, so
 * every sum over edges has one fixed order. No atomics, no host read. */
int ofx_motion_set_graph(void* handle, const ofx_motion_graph* g, ofx_stream_t s);
/* The network alone: pos f32 (N,3) centred positions, curr_motion f32 (N,4) [normalised motion | visible], hist f32
 * (T,N,4), 1 <= T <= 16 -> out f32 (N,4) = (mu, sigma), sigma after softplus; out 16-byte aligned. N must be the
 * graph's n[0] (else OFX_ERR_ARG; before ofx_motion_set_graph: OFX_ERR_STATE). 32 launches, two runs bitwise equal. */
int ofx_motion_forward(void* handle, const float* pos, const float* curr_motion, const float* hist, int32_t T,
                       int32_t n_nodes, float* out, ofx_stream_t s);
/* One frame of the runner: src / dst f64 (N,3) node positions at the source frame and at the tracked estimate, visible
 * u8 (N). Kabsch fit of the visible nodes (R the orthogonal polar factor of Hᵀ, no reflection fix), centimetres, std =
 * mean of the visible rows' per-axis std + 0.1, the history (cap max_hist, rescaled by std_prev / std, new nodes
 * appended as zeros, the previous-frame row from this call's and the last call's src), centred positions; the network;
 * confidence = exp(-conf_scale (sigma / (|mu| + 1))²), node_motion = mu std / 100 + rigid motion. Outputs: node_motion
 * f64 (N,3), confidence f64 (N), status i32 (1), and the network's inputs and raw output as they were used: pos_c f32
 * (N,3), curr_motion f32 (N,4), hist f32 (T',N,4) with T' = min(calls since reset, max_hist), raw f32 (N,4). status
 * bit 0: fewer than 3 visible nodes or a numerically singular H (|det H| <= 1e-12 |H|_F³): node_motion and confidence
 * are 0 for every node, the history is still advanced (with no rigid part); bit 1: the same for the previous-frame fit
 * (that history row then holds zero motion). N may grow between calls, never shrink (OFX_ERR_ARG). Stream-ordered,
 * no host read; the handle's state (history, last src and visible, std) lives on the device. */
int ofx_motion_complete(void* handle, const double* src, const double* dst, const uint8_t* visible, int32_t n_nodes,
                        double conf_scale, double* node_motion, double* confidence, int32_t* status, float* pos_c,
                        float* curr_motion, float* hist, float* raw, ofx_stream_t s);
/* Forget the history: the next ofx_motion_complete is a first call. The graph stays. */
int ofx_motion_reset(void* handle);
/* info i64[10]: launches of the last forward, history rows held, nodes of the last call, max_nodes, n[0..3] of the
 * graph (0 before ofx_motion_set_graph), max_hist, 0 */
int ofx_motion_info(void* handle, int64_t* info);

#ifdef __cplusplus
}
#endif
#endif /* OFX_H */
