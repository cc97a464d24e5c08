/*
 * yafaray_amd.h — MI355X extensions next to the drop-in ABI (yafaray_c_api.h).
 *
 * These entry points are additive (version node LIBYAFARAY_AMD_1.0): a reference client never
 * needs them.  They expose what a GPU host wants beyond the reference's per-pixel callbacks:
 *
 *  - bulk geometry upload (one call per object instead of one per vertex / triangle);
 *  - the batched ray-level seam that replaces the reference's per-ray const virtuals
 *    Accelerator::intersect / Accelerator::isShadowed (reference include/accelerator/accelerator.h:53-69,
 *    src/accelerator/accelerator.cc:55-78): SoA rays in, hits out, on the GPU BVH;
 *  - the rendered film (normalised RGBA + weights) as arrays, the in-kernel ray / node / triangle
 *    counters and per-phase timings the bench reports;
 *  - multi-GPU: render only a subset of tile rows (one process per GPU; the tile results are then
 *    all-gathered over RCCL by the caller).
 *
 * All pointers are plain host pointers unless a name says `_dev` (HIP device pointers, e.g. from
 * torch tensors on the same device).  Errors are reported the reference's way (logger + return 0).
 */
#ifndef YAFARAY_AMD_H
#define YAFARAY_AMD_H

#include "yafaray_c_api.h"
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct
{
	uint64_t closest_rays;      /* closest-hit queries issued to the BVH */
	uint64_t shadow_rays;       /* any-hit (shadow) queries */
	uint64_t node_visits;       /* BVH nodes fetched (64 B each) */
	uint64_t tri_tests;         /* triangles tested (48 B each) */
	uint64_t samples;           /* camera samples rendered */
	double build_seconds;       /* BVH build + upload (host) */
	double render_seconds;      /* GPU wall time of the sample loop + film (hipEvent) */
	double trace_kernel_ms;     /* summed k_trace time (hipEvent pairs), 0 if not profiled */
	uint64_t trace_launches;
	uint32_t bvh_nodes, bvh_depth, scene_in_lds, bvh_width;   /* bvh_width: children per node of the tree k_trace traverses (2, 4, or 8: the quantised BVH8) */
	uint32_t trace_grid, shade_grid;   /* persistent grids (workgroups) of k_trace / k_shade */
	uint32_t trace_block, stack_depth;
	double shade_kernel_ms;     /* summed k_shade time (hipEvent pairs), 0 if not profiled */
	double nee_kernel_ms;       /* summed k_nee time */
	uint64_t photons;           /* photons stored in the diffuse photon map (photon mapping) */
	double photon_seconds;      /* photon shooting + kd-tree build + upload */
	double photon_shoot_seconds, photon_tree_seconds;
	uint64_t gather_visits;     /* point kd-tree nodes fetched by the photon density estimates */
	uint64_t caustic_photons;   /* photons stored in the caustic photon map (0: none / disabled) */
	uint64_t radiance_points;   /* final gathering: radiance points picked while shooting */
	uint64_t radiance_photons;  /* final gathering: points kept (thinned) in the radiance map */
	double fg_thin_seconds;     /* final gathering: radiance-point thinning (host) incl. their download */
	double fg_radiance_seconds; /* final gathering: radiance map total (thinning, pre-gather, kd-tree) */
	int64_t fg_thin_rounds;     /* final gathering: GPU thinning rounds (-1: thinned on the host) */
	uint64_t gather_queries;    /* photon-map estimate requests k_gather served (1.2) */
	uint64_t gather_photons;    /* photon records the density estimates read (1.2) */
	int32_t photon_maps_mode;   /* photon_maps_processing the last render used after its fallbacks: 0 generate,
	                               1 generate-save, 2 load, 3 reuse-previous (1.2) */
	int32_t reserved0;
	uint64_t gather_accepts;    /* two-pass gather: photons the k_gather_walk logged (1.2) */
	uint64_t gather_overflows;  /* two-pass gather: requests whose log overflowed and were walked again (1.2) */
	uint64_t photon_paths_traced; /* photon shooting: path records the bounce launches traced, summed over bounces and maps (1.5) */
	uint64_t photon_slots;      /* photon shooting: deposit slots scanned by the compactions (paths x (bounces + 1)) (1.5) */
	uint64_t fg_paths;          /* final gathering: gather paths traced by k_fg (1.6) */
	uint64_t fg_lookups;        /* final gathering: radiance-map nearest searches (1.6) */
	uint64_t fg_nearest_visits; /* final gathering: radiance-map kd nodes those searches fetched (1.6) */
	uint64_t pregather_visits;  /* final gathering: diffuse-map kd nodes the radiance-map pre-gather fetched (1.6) */
	uint64_t pregather_photons; /* final gathering: photons summed by the pre-gather (1.6) */
	uint64_t pkd_split_level;   /* device / render group: the level at which the members split the last point kd-tree
	                               build (each built the subtrees below it it owns; 0 = every member built the whole tree) (1.6) */
} yafaray_amd_stats_t;

/* Bytes of the LIBYAFARAY_AMD_1.0 struct (its fields end at photon_tree_seconds): yafaray_amd_getStats
 * writes exactly these, so clients built against the 1.0 header keep working; newer clients call
 * yafaray_amd_getStatsEx with sizeof(yafaray_amd_stats_t). */
#define YAFARAY_AMD_STATS_V1_0_SIZE (offsetof(yafaray_amd_stats_t, gather_visits))
/* Bytes yafaray_amd_getStats@@LIBYAFARAY_AMD_1.4 (the default a client links against now) writes: every
 * field through fg_thin_rounds, which the header carried before getStatsEx existed.  Clients linked
 * against the 1.0 symbol keep receiving YAFARAY_AMD_STATS_V1_0_SIZE bytes. */
#define YAFARAY_AMD_STATS_V1_4_SIZE (offsetof(yafaray_amd_stats_t, gather_queries))

/* Bulk geometry: n vertices (xyz doubles, as addVertex) / n triangles (abc ints, as addTriangle). */
YAFARAY_C_API_EXPORT int yafaray_amd_addVertices(yafaray_Interface_t *interface, const double *xyz, int n);
YAFARAY_C_API_EXPORT yafaray_bool_t yafaray_amd_addTriangles(yafaray_Interface_t *interface, const int *abc, int n);

/* Build (or rebuild) the GPU acceleration structure for the current scene. */
YAFARAY_C_API_EXPORT yafaray_bool_t yafaray_amd_buildAccelerator(yafaray_Interface_t *interface);

/* Batched ray queries.  rays: n x 8 floats (from xyz, dir xyz, tmin, tmax; tmax < 0 = infinite).
 * closest: hits n x 1 float t (-1 = miss), prims n ints (global triangle index in creation order).
 * shadow : occluded n ints (Accelerator::isShadowed semantics: origin moved by tmin, t_max = tmax - 2 tmin). */
YAFARAY_C_API_EXPORT yafaray_bool_t yafaray_amd_traceClosest(yafaray_Interface_t *interface, const float *rays, int n, float *t, int *prims);
YAFARAY_C_API_EXPORT yafaray_bool_t yafaray_amd_traceShadow(yafaray_Interface_t *interface, const float *rays, int n, int *occluded);

/* Test infrastructure (LIBYAFARAY_AMD_1.9): the same queries through the kernel a render of this scene launches
 * (k_trace with its queues, per-segment counters, LDS stack levels, spill column and statistics), where
 * traceClosest / traceShadow run a plain traversal of their own.  The rays are dealt over n_seg queue segments
 * (1 <= n_seg <= the trace grid) with ragged counts; part: 0 both ray kinds, 1 closest only, 2 shadow only (the
 * launches of the overlapped schedule; the refill loops of scenes in global memory take 0 only).  A closest
 * ray whose direction x is NaN is the queue's "no ray" entry.  t, prims and occluded are in / out: entries
 * the kernel does not write keep the caller's values; a miss gets the kernel's own (prim -1, t = the ray's
 * tmax or infinity).  counted[0], counted[1]: the closest and shadow rays the launch's statistics report.
 * Statistics on / off follow yafaray_amd_setTraceStats.  False (and a logged error) for a scene without
 * accelerator, n_seg outside its range or a part the scene's kernel does not take. */
YAFARAY_C_API_EXPORT yafaray_bool_t yafaray_amd_traceQueued(yafaray_Interface_t *interface, const float *closest_rays, int n_closest,
                                                            const float *shadow_rays, int n_shadow, int n_seg, int part, float *t, int *prims,
                                                            int *occluded, unsigned long long *counted);

/* Test infrastructure (LIBYAFARAY_AMD_1.10): final gathering's radiance-point thinning on caller-supplied points.
 * pos, nrm: n x 3 floats; maxrad: the squared distance below which (strictly) two points whose normals face the
 * same side (dot > 0) are related.  kept (n entries of capacity) receives the kept indices in ascending order,
 * *n_kept their count.  mode 0: what a render does — the GPU rounds, or the host twin where the GPU refuses the
 * point set (its dense cell grid too large) or YAFARAY_AMD_FG_THIN=host asks for it; *rounds = the GPU's round
 * count, -1 after the host twin.  mode 1: the GPU only; false with a lastError text where it refuses.  mode 2:
 * the host twin only (no device needed).  Needs no scene; modes 0 and 1 run on the interface's device and stream
 * and reuse its thinning scratch from call to call. */
YAFARAY_C_API_EXPORT yafaray_bool_t yafaray_amd_thinRadPoints(yafaray_Interface_t *interface, const float *pos, const float *nrm, int n,
                                                              float maxrad, int mode, unsigned int *kept, int *n_kept, int *rounds);
/* Test infrastructure (LIBYAFARAY_AMD_1.11): the photon-map queries of a render on a caller-supplied map.
 * pos (and dir, for the nearest kinds): n x 3 floats; queries (and normals, nearest kinds): m x 3 floats.  The point
 * kd-tree is built by the production builder (YAFARAY_AMD_PKD_ORDER applies as in a render); every photon index
 * that comes back is an index into pos.  The m points become gather requests dealt over n_seg queue segments with
 * ragged counts (segment 0 empty when n_seg > 1) and run through the launches a render makes.  kind:
 *   0  what a render of this map would choose (k, YAFARAY_AMD_GATHER / _GATHER_HEAP / _GATHER_WALK / _GATHER_LOG);
 *      counters[7] names the path taken (1, 3, 4 or 5)
 *   1  the one-pass k_gather lookup            2  k_pregather's lookup
 *   3  k_gather_walk + packed-heap replay      4  k_gather_walk + split-heap replay (k <= 64 for both)
 *   5  the bounded walk + packed-heap replay (experiments builds only; where kind 0 takes this walk it replays with
 *      the heap a render would, the split one by default)
 *   6  pkNearest    7  the radiance grid (gridNearest; -2 = tie -> the kd search, as final gathering does)
 *   8  pkNearestLds (log_cap > 0: that many LDS stack levels instead of depth + 1; at most 32)
 * Gather kinds (0 - 5) search k photons within the squared radius radius2 and return per query: found, the final
 * squared radius, and the heap as the density estimate reads it, in heap-array order: heap_idx / heap_dist hold
 * k slots per query, the first found[q] set (the others 0xffffffff / 0).  log_cap: the walk's log entries per
 * request (even, >= k; 0 = a render's: max(k, YAFARAY_AMD_GATHER_LOG or 512) rounded up to even); a request that
 * accepts more overflows and is looked up again (counters[2]).  log_n (m) and log_e (m x log cap x 2 words: photon,
 * squared distance bits), both optional, receive the walk's raw log of kinds 0 and 3 - 5: log_n[q] entries were
 * accepted, the first min(log_n[q], cap) of them stored.
 * Nearest kinds search within radius2 for the nearest photon whose dir faces the query's normal (dot > 0):
 * nearest[q] = its index, -1 none.  Kind 7 also fills grid_raw (m) with gridNearest's own answer, -2 where it saw a
 * tie or no grid could be built (counters[10] = 0), and nearest holds the answer after the kd search settled those.
 * counters (16 values): 0 kd nodes visited, 1 photons the walk accepted, 2 requests whose log overflowed, 3 the
 * tree's deepest level (root 0), 4 pm_stack (depth + 1), 5 the stack levels kept in LDS (walk kinds, kind 8),
 * 6 whether the walk got a spill column for deeper levels, 7 the path, 8 the largest n_seg allowed, 9 the log cap
 * used, 10 whether the grid was built, 11 queries the grid answered -2, 12 photons found in all, 13 whether the
 * leaves are in kd order.  False with a lastError text, and nothing launched, for n <= 0, k < 1, m < 0, n_seg
 * outside [1, counters[8]], an odd or negative log_cap, log_cap below k, a kind this build does not have, or
 * missing arrays.  Needs no scene; runs on the interface's device and stream with buffers of its own. */
YAFARAY_C_API_EXPORT yafaray_bool_t yafaray_amd_queryPhotons(yafaray_Interface_t *interface, const float *pos, const float *dir, int n,
                                                             const float *queries, const float *normals, int m, int k, float radius2, int n_seg,
                                                             int log_cap, int kind, int *found, float *radius2_out, unsigned int *heap_idx,
                                                             float *heap_dist, int *nearest, int *grid_raw, unsigned int *log_n,
                                                             unsigned int *log_e, unsigned long long *counters);
/* Test infrastructure (LIBYAFARAY_AMD_1.10): adaptive anti-aliasing's nextPass on a caller-supplied accumulated film.
 * accum: width x height x 4 floats (unnormalised), weights: width x height; tile: the tile size of the visiting
 * order; detect_color_noise ... variance_pixels: the AA noise parameters (dark_type 0 none, 1 linear, 2 curve);
 * rows [ry0, ry1): the band whose resampled pixels are listed.  flags (width x height bytes) receives the whole
 * film's resample flags, *count their number, plist (width x height entries of capacity) the flagged pixels
 * (y * width + x) of the band in visiting order, *local_count how many.  False (and a logged error, nothing
 * launched) for width, height or tile <= 0 or a row range outside 0 <= ry0 <= ry1 <= height.  Needs no scene. */
YAFARAY_C_API_EXPORT yafaray_bool_t yafaray_amd_aaNextPass(yafaray_Interface_t *interface, const float *accum, const float *weights, int width,
                                                           int height, int tile, int detect_color_noise, int dark_type, float dark_factor,
                                                           int variance_edge, int variance_pixels, float threshold, int ry0, int ry1,
                                                           unsigned char *flags, unsigned int *plist, unsigned int *count,
                                                           unsigned int *local_count);

/* The built scene's primitives [first, first + count) in creation order (instances expanded, as the
 * ray queries number them), as the device holds them: verts9 the three world-space vertices, ng3 the
 * geometric normal, vnormals9 the three vertex normals (the geometric normal where the primitive is
 * not smooth), material the material's creation index.  Any output may be NULL.  Builds the scene if
 * it is dirty; count = 0 with every output NULL only builds.  Returns the scene's primitive count,
 * -1 on failure. */
YAFARAY_C_API_EXPORT int yafaray_amd_getPrimitives(yafaray_Interface_t *interface, int first, int count, float *verts9, float *ng3, float *vnormals9, int *material);

/* Film of the last render: rgba width*height*4 floats (normalised, = put-pixel values), weights width*height. */
YAFARAY_C_API_EXPORT yafaray_bool_t yafaray_amd_getFilm(const yafaray_Interface_t *interface, float *rgba, float *weights);
/* Render layers (LIBYAFARAY_AMD_1.8).  yafaray_defineLayer accepts, beside "combined", the first-hit layers
 * z-depth-abs, z-depth-norm, mist, debug-normal-geom, debug-normal-smooth, debug-uv, debug-barycentric-uvw,
 * adv-diffuse-color, obj-index-abs, obj-index-norm, mat-index-abs and mat-index-norm; every other type
 * warns and is not produced.
 * getLayerCount: the layers the next render produces, "combined" included (0 without a scene).
 * getLayerName: layer k's type name in the reference's layer order ("combined" first); NULL out of range.
 *   The string lives until the scene's layers change. */
YAFARAY_C_API_EXPORT int yafaray_amd_getLayerCount(const yafaray_Interface_t *interface);
YAFARAY_C_API_EXPORT const char *yafaray_amd_getLayerName(const yafaray_Interface_t *interface, int k);
/* One layer of the last render's film: rgba width*height*4 floats, the values put-pixel reports for the
 * layer — normalised, ceil() of the absolute index layers, alpha 1 for an image type without alpha.
 * Also serves layers defined without exported_image_type (no callbacks).  False: no such layer rendered. */
YAFARAY_C_API_EXPORT yafaray_bool_t yafaray_amd_getFilmLayer(const yafaray_Interface_t *interface, const char *layer, float *rgba);
/* Film straight into device memory (rows [y0, y1) of a width*height*4 float buffer on the render device). */
YAFARAY_C_API_EXPORT yafaray_bool_t yafaray_amd_getFilmDevice(const yafaray_Interface_t *interface, void *rgba_dev, int y0, int y1);

/* Restrict the next render to tile rows r with r % world == rank (one process per GPU).  world = 1 renders all. */
YAFARAY_C_API_EXPORT void yafaray_amd_setTileRowShard(yafaray_Interface_t *interface, int rank, int world);
/* Restrict the next render to the contiguous pixel-row band [height*rank/world, height*(rank+1)/world)
   (the default split across GPUs: per-row cost is nearly uniform; one halo row is rendered twice). */
YAFARAY_C_API_EXPORT void yafaray_amd_setRowBandShard(yafaray_Interface_t *interface, int rank, int world);
/* Restrict the next render to the explicit pixel-row band [y0, y1) of a film split over `world` GPUs
   (host-side load balancing moves the band boundaries between frames; halo rows are added here). */
YAFARAY_C_API_EXPORT void yafaray_amd_setRowBandRange(yafaray_Interface_t *interface, int y0, int y1, int world);
/* Pixel-row ranges [rows[2k], rows[2k+1]) owned by this rank in the last render; returns their count
   (at most max_ranges are written). */
YAFARAY_C_API_EXPORT int yafaray_amd_getOwnedRows(const yafaray_Interface_t *interface, int *rows, int max_ranges);

/* Render without callbacks / console output (bench loop); same work as yafaray_render. */
YAFARAY_C_API_EXPORT yafaray_bool_t yafaray_amd_renderQuiet(yafaray_Interface_t *interface);

/* Counters and timings of the last render: YAFARAY_AMD_STATS_V1_4_SIZE bytes (a client linked against the
 * LIBYAFARAY_AMD_1.0 version of this symbol: YAFARAY_AMD_STATS_V1_0_SIZE bytes). */
YAFARAY_C_API_EXPORT void yafaray_amd_getStats(const yafaray_Interface_t *interface, yafaray_amd_stats_t *stats);
/* (LIBYAFARAY_AMD_1.2) All counters: copies min(bytes, sizeof(yafaray_amd_stats_t)) bytes, returns how many. */
YAFARAY_C_API_EXPORT size_t yafaray_amd_getStatsEx(const yafaray_Interface_t *interface, yafaray_amd_stats_t *stats, size_t bytes);

/* Per-kernel timing of the last render with setProfileKernels on (HIP events before / after every
 * launch on the render stream): for each kernel kind k < return value (and < max): its name, summed
 * launch time in ms, launch count and work items (samples for k_camera / k_film, rays for k_trace,
 * active entries for k_shade, requests for k_nee, queries for k_gather, photon paths for the photon
 * shoot, stored photons for the photon map).  Any output pointer may be NULL.  (LIBYAFARAY_AMD_1.1) */
YAFARAY_C_API_EXPORT int yafaray_amd_getKernelTimes(const yafaray_Interface_t *interface, const char **names, double *ms, uint64_t *launches,
                                                    uint64_t *items, int max);

/* Render group (LIBYAFARAY_AMD_1.1): several GPUs render one film, one member per GPU (e.g. one
 * process per GPU).  Member 0 creates the group id (an RCCL unique id, <= 128 bytes) and hands it to
 * the others by any host means; every member then calls setRenderGroup with its rank on its own
 * current HIP device.  From then on yafaray_render / renderQuiet on each member renders a contiguous
 * band of pixel rows (+ the halo rows its splats need) and all-gathers every band over RCCL (xGMI)
 * into the member's film: each member ends with the whole frame, bit-identical to a one-GPU render.
 * The bands follow the members' measured render times from frame to frame (rebalanceBands).
 * world = 1 leaves the group.  getRenderGroupId returns the id size (0 on failure). */
YAFARAY_C_API_EXPORT int yafaray_amd_getRenderGroupId(void *id, int bytes);
YAFARAY_C_API_EXPORT yafaray_bool_t yafaray_amd_setRenderGroup(yafaray_Interface_t *interface, int rank, int world, const void *id, int bytes);
/* Device group (LIBYAFARAY_AMD_1.2): ONE process renders one film on several GPUs — one member per
 * GPU, each on its own host thread and HIP stream, rendering a contiguous row band (+ halo rows);
 * the members exchange the accumulated film between adaptive passes and member 0 pulls every band
 * over xGMI at the end, so the film is bit-identical to a one-GPU render.  By default the group is
 * every visible device (render parameter "gpus": -1 = all, n = the first n devices starting at the
 * current one; env YAFARAY_AMD_GPUS overrides), so an unmodified reference client's yafaray_render
 * uses the whole node.  setDeviceGroup fixes the members explicitly: devices[m] is member m's HIP
 * device (devices NULL: the current device + m, modulo the visible devices — several logical members
 * may share one GPU, which rehearses the group on one device); members <= 0 returns to "gpus".
 * A render group (setRenderGroup) always renders with one member per process. */
YAFARAY_C_API_EXPORT yafaray_bool_t yafaray_amd_setDeviceGroup(yafaray_Interface_t *interface, int members, const int *devices);
/* Members the next render uses (0 on failure, e.g. no GPU). */
YAFARAY_C_API_EXPORT int yafaray_amd_getDeviceGroupSize(yafaray_Interface_t *interface);

/* The group's band balancer: world + 1 boundaries and each band's render time -> new boundaries
 * (out, world + 1 ints); cap_rows > 0 rejects a split with a larger band.  Returns 1. */
YAFARAY_C_API_EXPORT int yafaray_amd_rebalanceBands(const int *bounds, int world, const double *times, int cap_rows, int *out);

/* (LIBYAFARAY_AMD_1.2) The render group's band exchange plan on host arrays, as the group runs it on
 * device buffers: packBand writes member `rank`'s rows [bounds[rank], bounds[rank+1]) of a
 * width x height x channels film into a zero-padded slot of the largest band's rows; after an
 * all-gather of the slots (member order), unpackBands copies every other member's rows into the
 * film.  Return 1 (0: bad arguments). */
YAFARAY_C_API_EXPORT int yafaray_amd_packBand(const float *film, int width, int height, int channels, const int *bounds, int world, int rank,
                                              float *send);
YAFARAY_C_API_EXPORT int yafaray_amd_unpackBands(const float *recv, int width, int height, int channels, const int *bounds, int world,
                                                 int rank, float *film);

/* Tuning: samples in flight per wavefront chunk (default 1 << 25, halved automatically if it does not fit) and whether to time k_trace with events. */
/* (LIBYAFARAY_AMD_1.3) The photon map's point kd-tree on its own (batched seam for
 * PointKdTree<T>::PointKdTree, reference include/photon/pkdtree.h:115-222): n positions (x, y, z) in,
 * 2n - 1 nodes of 4 uint32 out in the reference's depth-first layout (.w: bits 0-1 axis or 3 = leaf,
 * interior: right child << 2 and .x the split position bits, .y / .z the parent's plane; leaf:
 * photon index << 2 and .xyz its position bits), *depth = deepest level (root 0).  Current device. */
YAFARAY_C_API_EXPORT yafaray_bool_t yafaray_amd_buildPhotonTree(const float *xyz, int n, unsigned int *nodes, int *depth);
/* (LIBYAFARAY_AMD_1.6) The distributed build of a device / render group (what a group render runs for its
 * photon maps): member `member` of `members` builds the levels above *split_level = ceil(log2 members)
 * (0: too few photons to split — the whole tree) and the level-D subtrees it owns, with the map's records
 * in kd order (leaves index kd_pos, n x 4 floats); the other members' subtrees and the parent planes
 * (.y / .z of interior nodes) are left zero — a group exchanges the ranges yafaray_amd_photonTreeSegments
 * gives and writes the planes.  *ms = the build's device time (second of two builds).  Current device. */
YAFARAY_C_API_EXPORT yafaray_bool_t yafaray_amd_buildPhotonTreeMember(const float *xyz, int n, int member, int members, unsigned int *nodes,
                                                                      float *kd_pos, int *depth, int *split_level, double *ms);
/* (LIBYAFARAY_AMD_1.6) The level-`level` subtrees of a tree over n photons, (node, start, end) each in
 * segments[3 << level] (nodes [node, node + 2 (end - start) - 1), kd-order records [start, end)), and the
 * consecutive ones member `member` of `members` owns: [*s0, *s1). */
YAFARAY_C_API_EXPORT void yafaray_amd_photonTreeSegments(unsigned int n, int level, int member, int members, unsigned int *segments,
                                                         unsigned int *s0, unsigned int *s1);
YAFARAY_C_API_EXPORT void yafaray_amd_setChunkSlots(yafaray_Interface_t *interface, int slots);
YAFARAY_C_API_EXPORT void yafaray_amd_setProfileKernels(yafaray_Interface_t *interface, yafaray_bool_t enable);
/* (LIBYAFARAY_AMD_1.2) Per-visit BVH node / triangle counters in the traversal kernels (default on).
 * Off: the stats report rays only (node_visits / tri_tests stay 0) and k_trace runs ~1-2% faster. */
YAFARAY_C_API_EXPORT void yafaray_amd_setTraceStats(yafaray_Interface_t *interface, yafaray_bool_t enable);

/* Diagnostic: summed wave cycles of the k_shade phases (load, connect, hit, next segment, compaction,
 * NEE) since the last reset; returns the number of counters, 0 unless the library was built with
 * -DYAF_PHASE_TIMING (never in the product build). */
YAFARAY_C_API_EXPORT int yafaray_amd_getPhaseCycles(unsigned long long *cycles, int n, yafaray_bool_t reset);

/* (LIBYAFARAY_AMD_1.4) The library's build: the device objects' architecture and extra compile flags
 * (a variant build, e.g. -DYAF_PHASE_TIMING, shows here) and the host compiler.  Static storage. */
YAFARAY_C_API_EXPORT const char *yafaray_amd_buildInfo(void);
/* (LIBYAFARAY_AMD_1.4) How the last render was split across GPUs, as one JSON object: "mode" ("one GPU",
 * "device group", "render group"), "members", "devices", the hipDeviceCanAccessPeer matrix over this
 * process's distinct member devices ("peer_devices", "peer_access"), "copy_path" (how the bands
 * travel), "bounds" (the row-band boundaries the render used), "member_ms" (each member's render time)
 * and "next_bounds" (the rebalanced boundaries of the next frame).  Writes at most bytes - 1 characters
 * + NUL into buf (may be NULL) and returns the length the whole report needs, NUL included (0: no scene). */
YAFARAY_C_API_EXPORT size_t yafaray_amd_getGroupReport(yafaray_Interface_t *interface, char *buf, size_t bytes);

/* Last error message (empty if none); owned by the interface. */
YAFARAY_C_API_EXPORT const char *yafaray_amd_lastError(const yafaray_Interface_t *interface);

#ifdef __cplusplus
}
#endif

#endif /* YAFARAY_AMD_H */
