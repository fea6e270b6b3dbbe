/* C ABI of libpswin_poly_hip.so: COCO polygon annotations to masks on the device (csrc/pswin_poly.hip;
 * panoswintransformerobjectdetection_amd/polygons.py states the rule, pycocotools' rleFrPoly, and holds the definitions:
 * rle_from_polygon, PolygonBatch, polygons_to_masks, polygons_to_rle).  A library of its own beside libpswin_hip.so (include/pswin.h),
 * whose status codes it shares; gfx950 only. */
#ifndef PSWIN_POLY_H
#define PSWIN_POLY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSWIN_POLY_ABI_VERSION 1
int pswin_poly_version(void);

/* xy f64 [max_vertices][2] (x, y), 16-byte aligned; part_offsets int32 [max_parts + 1]: part p owns the vertices part_offsets[p] ..
 * part_offsets[p + 1]; obj_offsets int32 [B K + 1]: object n = b K + k owns the parts obj_offsets[n] .. obj_offsets[n + 1]; count int32
 * [B]: an object is read only when k < count[b] clamped to [0, K].  All on the device; every offset is clamped to its buffer before it
 * is used, and the work per edge is bounded whatever the coordinates are (a comparison, or at most 24 bisection steps), so stale
 * buffers are read in bounds and cost no more than their size.
 * pswin_poly_masks writes every byte of masks uint8 [B K][H][W]: 0 / 1, the OR of the object's parts, zeros for the objects past a
 * count.  Two launches (polygons -> bit-planes in the workspace, planes -> bytes with 16-byte stores where W % 16 == 0 and masks is
 * 16-byte aligned); fixed shapes, no atomics, no cursor, no host synchronisation: the output is a function of the inputs alone and the
 * call can be captured.  Arguments are validated before the device is touched (PSWIN_ERR_ARG).  Limits: H, W <= 4096, B K < 2^31.
 * workspace: pswin_poly_workspace bytes (8 B K ceil(H / 64) W), 16-byte aligned; every part of it is written before it is read. */
int pswin_poly_workspace(int B, int K, int H, int W, long long* bytes);
int pswin_poly_masks(const double* xy, const int32_t* part_offsets, const int32_t* obj_offsets, const int32_t* count, int max_parts,
                     int max_vertices, int B, int K, int H, int W, unsigned char* masks, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif
