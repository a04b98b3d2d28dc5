/* vgicp_hip_search_report.h — extension of the C ABI (vgicp_hip.h): a developer's test hook, like vgicp_solve_step
 * and vgicp_voxel_index: which paths the neighbour search of the last scan preparation took.
 *
 * The exact k-nearest-neighbour search of the scan preparation (knn_search_kernel, eskf_lio_amd/csrc/
 * vgicp_preprocess.hip) reaches its result through many routes: a home cell or none, a 27-cell block at a level chosen
 * from the first bound, cells opened one or two levels down or measured as leaves, a pool of waiting cells that is
 * compacted and spilled, a candidate buffer whose bound a radix select tightens, an all-pairs ranking when the select
 * cannot tell the candidates apart, a sweep over the whole scan.  Every route returns the same neighbours; a test of
 * one of them has to know that it ran.  A context created with VGICP_DEBUG_PREP set (to 1 or more) counts, per
 * preparation, the queries that took each path; this call reads the counts.
 *
 * Declared here and not in vgicp_hip.h: the main header's list of entry points is pinned.  The function is defined
 * in a library of its own beside the module, libvgicp_hip_search_report.so, which links against libvgicp_hip.so. */
#ifndef VGICP_HIP_SEARCH_REPORT_H_
#define VGICP_HIP_SEARCH_REPORT_H_

#include "vgicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 96 bytes.  Every count but the two maxima is a number of queries (one query per kept point). */
typedef struct vgicp_search_report {
  uint32_t kept;             /* kept points = queries of the search */
  uint32_t n_heavy;          /* queries of sparse neighbourhoods: the start list that is dispatched first */
  uint32_t n_light;          /* the others: the start list dealt over the XCDs behind them */
  /* -- everything below: only from a context created with VGICP_DEBUG_PREP -- */
  uint32_t cells;            /* octree cells over all levels */
  uint32_t spilled_or_swept; /* queries with a spill or a whole-scan sweep (the stderr line's "queries that spilled") */
  uint32_t batches_total;    /* batches of up to 64 points measured, all queries */
  uint32_t batches_max;      /* ... the most by one query */
  uint32_t cells_total;      /* waiting cells taken, all queries */
  uint32_t cells_max;        /* ... the most by one query */
  uint32_t above_voxel;      /* queries whose 27-cell block is coarser than the voxel level */
  /* the fourteen paths: queries that ... */
  uint32_t home;             /* started from their own cell (the finest that holds k points, at most 128) */
  uint32_t crowded;          /* have such a cell, but it holds more than 128 points: no home */
  uint32_t no_own_cell;      /* have no own cell with k points on any level */
  uint32_t window_is_k;      /* opened with exactly k candidates: the bound is their largest distance */
  uint32_t whole_scan;       /* no level's 27-cell block covers the first bound: every point of the scan measured */
  uint32_t clipped;          /* sit where the 27-cell block reaches over the edge of the search grid */
  uint32_t open2;            /* opened a cell two levels down */
  uint32_t open1;            /* opened a level-1 cell one level down */
  uint32_t leaf;             /* measured a cell above the finest level */
  uint32_t finest;           /* measured a finest cell */
  uint32_t compacted;        /* compacted their pool of waiting cells */
  uint32_t spilled;          /* found no room in the pool even so and measured the cell instead of opening it */
  uint32_t waited;           /* had candidates of one batch wait for room in the 64-entry buffer */
  uint32_t reranked;         /* kept more than 56 candidates after a select: exact all-pairs ranking */
} vgicp_search_report;

/* Fills *report from the last preparation of a single-device context that has been settled (vgicp_preprocess,
 * vgicp_scan_prepare, or an enqueued preparation once a later call has settled it; a pending one is settled here).
 *   - ctx or report NULL, a context of another build of the module, a multi-device context: VGICP_ERR_BAD_ARGUMENT;
 *   - no preparation has been settled yet, or the last one was refused: VGICP_ERR_NOT_READY, *report zeroed;
 *   - a context created without VGICP_DEBUG_PREP: kept, n_heavy and n_light are filled, the rest is zero, and the
 *     call returns VGICP_ERR_BAD_ARGUMENT (the counts do not exist: production searches write none);
 *   - else VGICP_OK. */
int vgicp_prepare_search_report(vgicp_ctx* ctx, vgicp_search_report* report);

#ifdef __cplusplus
}
#endif

#endif /* VGICP_HIP_SEARCH_REPORT_H_ */
