// The launch API: every extern "C" yafamd_* function that host code calls across a file boundary, grouped by the
// unit that defines it.  The host files that call them (render.cc, c_api.cc) and every .hip that defines one
// include this header, so a definition whose parameter list disagrees with its declaration is a compile error
// instead of a call that links and reads shifted arguments.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "bvh.h"
#include "devscene.h"

extern "C" {

// kernels.hip
hipError_t yafamd_launch_camera(const yafamd::DevScene *S, const yafamd::DevPaths *P, const yafamd::DevQueues *Q, const yafamd::DevCounters *cnt,
                                const yafamd::DevJob *jobs, int n_jobs, uint64_t chunk_base, int n, int write_pr, hipStream_t st);
hipError_t yafamd_launch_surface(const yafamd::DevScene *S, const yafamd::DevQueues *Q, const yafamd::DevCounters *cnt, hipStream_t st);
hipError_t yafamd_launch_tshadow(const yafamd::DevScene *S, const yafamd::DevQueues *Q, const yafamd::DevCounters *cnt, const yafamd::DevPaths *P, hipStream_t st);
hipError_t yafamd_launch_spawn(const yafamd::DevScene *S, const yafamd::DevPaths *P, const yafamd::DevQueues *Q, const yafamd::DevCounters *cnt, uint32_t s0, int n,
                               hipStream_t st);
hipError_t yafamd_launch_combine(const yafamd::DevScene *S, uint32_t lo, uint32_t hi, int final_level, float4 *samples, const yafamd::DevJob *jobs,
                                 int n_jobs, uint64_t chunk_base, hipStream_t st);
hipError_t yafamd_launch_trace(const yafamd::DevScene *S, const yafamd::DevQueues *Q, const yafamd::DevCounters *cnt, const yafamd::DevPaths *P,
                               yafamd::DevStats *stats, int stack_depth, int *spill, const float4 *flat_tab, int grid, hipStream_t st);
int yafamd_trace_block();
int yafamd_shade_fused();
unsigned long long yafamd_xl_launches();
int yafamd_walk_lds_levels(int pm_stack);
int yafamd_walk_threads(const yafamd::DevScene *S);
int yafamd_shade_fused_for(const yafamd::DevScene *S);
int yafamd_experiments();
int yafamd_trace_blocks_per_cu(int lds_scene, int wide, size_t dyn_lds, int defer);
int yafamd_trace_defer_ok(int n_tris, int max_leaf);
int yafamd_trace_defer_min_cap();
int yafamd_shade_blocks_per_cu();
hipError_t yafamd_launch_shade(const yafamd::DevScene *S, const yafamd::DevPaths *Pc, const yafamd::DevPaths *Pn, const yafamd::DevQueues *Q,
                               const yafamd::DevQueues *Qn, const yafamd::DevNeeQueue *N, const yafamd::DevNeeQueue *G, const yafamd::DevCounters *cnt,
                               const yafamd::DevCounters *cnt_next, float4 *samples, const yafamd::DevJob *jobs, int n_jobs, uint64_t chunk_base,
                               int stage_it, hipStream_t st);
int yafamd_shade_stages_for(const yafamd::DevScene *S);
int yafamd_shade_stage_errors(uint32_t *out, int n);
int yafamd_path_eligible(const yafamd::DevScene *S, int stack_depth, int spill);
int yafamd_path_blocks_per_cu(const yafamd::DevScene *S, int stack_depth);
hipError_t yafamd_launch_path(const yafamd::DevScene *S, float4 *samples, const yafamd::DevJob *jobs, int n_jobs, uint64_t chunk_base, uint32_t n,
                              uint32_t *next, int stack_depth, int grid, hipStream_t st);
hipError_t yafamd_launch_nee(const yafamd::DevScene *S, const yafamd::DevNeeQueue *N, const yafamd::DevPaths *Pn, const yafamd::DevQueues *Qn,
                             const yafamd::DevCounters *cnt_next, int stack_depth, hipStream_t st);
int yafamd_nee_blocks_per_cu();
hipError_t yafamd_photon_emit(const yafamd::DevScene *S, const yafamd::PhotonState *P, const yafamd::PhotonSet *L, uint32_t n_photons, uint32_t h0, uint32_t n_local,
                              int max_bounces, hipStream_t st);
hipError_t yafamd_photon_bounce(const yafamd::DevScene *S, const yafamd::PhotonState *P, const yafamd::PhotonSet *L, uint32_t n_photons, uint32_t h0,
                                uint32_t n_local, int max_bounces, int bounce, int cur, int stack_depth, int *spill, int grid, hipStream_t st);
hipError_t yafamd_photon_compact(const yafamd::PhotonState *P, uint32_t *scratch_counts, uint32_t *total_dev, float4 *pos, float4 *dir, float *colb,
                                 hipStream_t st);
hipError_t yafamd_launch_gather(const yafamd::DevScene *S, const yafamd::DevNeeQueue *G, const yafamd::DevCounters *cnt_next, float4 *samples,
                                const yafamd::DevJob *jobs, int n_jobs, uint64_t chunk_base, const yafamd::GatherLogDesc *log, hipStream_t st,
                                uint32_t *probe_out = nullptr);
hipError_t yafamd_launch_gather_walk(const yafamd::DevScene *S, const yafamd::DevNeeQueue *G, const yafamd::DevCounters *cnt_next, const yafamd::GatherLogDesc *log,
                                     hipStream_t st);
int yafamd_gather_walk_k();
int yafamd_walk_exact_k();
size_t yafamd_gather_lds_bytes(const yafamd::DevScene *S);
hipError_t yafamd_rad_compact(const yafamd::PhotonState *P, uint32_t *scratch_counts, uint32_t *total_dev, float4 *a, float4 *b, float4 *c, hipStream_t st);
hipError_t yafamd_rad_refl(const yafamd::DevScene *S, float4 *a, float4 *b, float4 *c, const uint32_t *kept, uint32_t n, hipStream_t st);
hipError_t yafamd_pregather(const yafamd::DevScene *S, const float4 *a, const float4 *b, const float4 *c, const uint32_t *kept, uint32_t n,
                            float4 *out_pos, float4 *out_dir, float *out_colb, yafamd::DevStats *stats, hipStream_t st, uint32_t *probe_out = nullptr);
// (test infrastructure, yafaray_amd_queryPhotons) the nearest searches on caller-supplied points
hipError_t yafamd_nearest_probe(const uint4 *nodes, const float4 *dirs, const yafamd::RadGrid *grid, const float4 *qp, const float4 *qn, uint32_t m,
                                float max_d2, int mode, int cap, int *out, int *out_grid, unsigned long long *visits, hipStream_t st);
int yafamd_fg_paths_eligible(const yafamd::DevScene *S);
hipError_t yafamd_launch_fg_paths(const yafamd::DevScene *S, const yafamd::DevNeeQueue *G, const yafamd::DevCounters *cnt_next, int stack_depth, int *spill, int grid,
                                  const yafamd::FgBatch *B, hipStream_t st);
int yafamd_dfr_eligible(const yafamd::DevScene *S);
hipError_t yafamd_dfr_segoff(const yafamd::DevCounters *cnt, uint32_t n_seg, uint32_t *seg_off, uint32_t *dfr_total, uint32_t cap, uint32_t *overflow,
                             uint32_t *it_start, hipStream_t st);
hipError_t yafamd_dfr_accum(const yafamd::DevScene *S, const yafamd::DevPaths *P, uint32_t r0, uint32_t r1, uint32_t batch0, float4 *pcol, hipStream_t st);
hipError_t yafamd_dfr_nee(const yafamd::DevScene *S, const yafamd::DevPaths *P, const yafamd::DevQueues *Q, const yafamd::DevCounters *cnt, uint32_t r0, uint32_t total, uint32_t *idx,
                         uint32_t *n_rec, hipStream_t st);
hipError_t yafamd_dfr_fold(const yafamd::DevScene *S, float4 *samples, uint32_t n_ctr, const float4 *pcol, hipStream_t st);
hipError_t yafamd_launch_fg(const yafamd::DevScene *S, const yafamd::DevNeeQueue *G, const yafamd::DevCounters *cnt_next, int stack_depth, int *spill, int grid, float2 *ts_scratch,
                            hipStream_t st);
size_t yafamd_gather_lanes(const yafamd::DevScene *S);
hipError_t yafamd_launch_trace_rays(const yafamd::DevScene *S, int any, const float4 *ro, const float4 *rd, int n, float *t_out,
                                    int *prim_out, int stack_depth, hipStream_t st);
int yafamd_phase_cycles(unsigned long long *out, int n, int reset);
const char *yafamd_device_build();

// film.hip
hipError_t yafamd_launch_done_flags(const yafamd::DevScene *S, const yafamd::DevJob *jobs, int n_jobs, uint32_t n_pix, uint32_t done_pix, uint8_t *flags,
                                    hipStream_t st);
hipError_t yafamd_lpc_seg(const uint32_t *lpc, int W, int spp, int ts, int y0, int y1, uint32_t *seg, hipStream_t st);
hipError_t yafamd_lpc_prefix(uint32_t *lpc, int W, int spp, int ts, int y0, int y1, const uint32_t *segbase, hipStream_t st);
hipError_t yafamd_launch_film(const yafamd::DevFilm *F, const float4 *samples, const uint8_t *flags, float4 *accum, float4 *out,
                              float *weights, int y0, int y1, float clamp_samples, int accumulate, hipStream_t st);

// layers.hip
hipError_t yafamd_layer_depth_range(const yafamd::DevScene *S, float *range, int stack_depth, hipStream_t st);
hipError_t yafamd_launch_layer_hits(const yafamd::DevScene *S, const yafamd::DevLayers *L, const yafamd::DevJob *jobs, int n_jobs, uint64_t chunk_base, int n, int stack_depth,
                                    hipStream_t st);
hipError_t yafamd_launch_layer_film(const yafamd::DevFilm *F, const yafamd::DevLayers *L, const float4 *prim_ng, const uint8_t *flags, float4 *accum, float4 *out,
                                    const float *weights, int y0, int y1, float clamp_samples, int accumulate, hipStream_t st);

// pkd.hip
hipError_t yafamd_build_pkd(const float4 *pos_dev, uint32_t n, uint4 *nodes_dev, int *depth_out, hipStream_t st, void **scratch);
hipError_t yafamd_build_pkd_kd(const float4 *pos_dev, const float4 *dir_dev, const float *colb_dev, uint32_t n, uint4 *nodes_dev, float4 *kpos,
                               float4 *kdir, float *kcolb, int *depth_out, hipStream_t st, void **scratch);
void yafamd_pkd_scratch_free(void *scratch);
hipError_t yafamd_build_pkd_kd_member(const float4 *pos_dev, const float4 *dir_dev, const float *colb_dev, uint32_t n, uint4 *nodes_dev, float4 *kpos,
                                      float4 *kdir, float *kcolb, int *depth_out, hipStream_t st, void **scratch, int member, int members,
                                      int *split_level);
void yafamd_pkd_top_segments(uint32_t n, int level, uint32_t *out);
void yafamd_pkd_owned_segments(int level, int member, int members, uint32_t *s0, uint32_t *s1);
hipError_t yafamd_pkd_parent_planes(uint4 *nodes_dev, uint32_t n, hipStream_t st);

// aa.hip
hipError_t yafamd_aa_next_pass(const float4 *accum, const float *weights, int W, int H, int tile, const yafamd::DevAaParams *prm,
                               float threshold, uint8_t *flags, uint32_t *plist, uint32_t *count, int ry0, int ry1, uint32_t *local_count,
                               hipStream_t st);

// fgthin.hip
hipError_t yafamd_thin_rad_points(const float4 *pos, const float4 *nrm, uint32_t n, float maxrad, uint32_t *kept_out, uint32_t *n_kept,
                                  int *rounds_out, hipStream_t st, void **scratch);
void yafamd_thin_scratch_free(void *scratch);
hipError_t yafamd_rad_grid(const float4 *pos, const float4 *dir, uint32_t n, float lookup_rad, yafamd::RadGrid *out, hipStream_t st, void **scratch);
void yafamd_rad_grid_free(void *scratch);

// bvhgpu.hip
hipError_t yafamd_ray_bin(const yafamd::DevQueues *Q, const yafamd::DevCounters *cnt, uint32_t n_seg, uint32_t cap_a, const float *lo, const float *hi,
                          uint32_t *keys_in, uint32_t *keys_out, uint32_t *iota, uint32_t *perm, void *tmp, size_t *tmp_bytes, hipStream_t st);
hipError_t yafamd_build_bvh_gpu(const float *verts_dev, const int *tris_dev, int n, void **nodes_out, void **tris_out,
                                int *n_nodes, int *depth, int *stack_need, int *ploc_iters, yafamd::YafBvh8 *w8, hipStream_t st);

// instexpand.hip
hipError_t yafamd_instance_expand(const yafamd::DevInstSeg *segs, int n_segs, const float *src_verts, const int *src_tris, const float4 *src_ng,
                                  const float4 *src_attr, int n_out_verts, int n_out_prims, float *out_verts, int *out_tris, float4 *out_ng,
                                  float4 *out_attr, float *bounds, hipStream_t st);

}
