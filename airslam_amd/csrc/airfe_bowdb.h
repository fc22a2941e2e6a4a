// airfe — the keyframe database behind the opaque airfe_bowdb pointer (include/airfe.h "BoW keyframe database"), shared by airfe_bowdb.hip, airfe_bowmap.hip and
// airfe_junction.hip: the struct, the accessor of its row tables and the *_queue functions more than one of the files queues.
#pragma once
#include "airfe_host.h"

// Every device array lives in a DevBlock.  The persistent tables' blocks are reserved once (create, attach_map, attach_point_ids) and never grown; their typed
// pointers are set once the block is there.  airfe_bowdb_destroy hands all blocks back as one list.
struct airfe_bowdb {
  airfe_ctx* c = nullptr;
  int max_frames = 0, cap = 0, keep = 0, size = 0;
  DevBlock tables[5];                                                        // create: the next two lines, a block each (profiles/r29_bowdb_host_ab.txt)
  uint32_t* ids = nullptr; double* vals = nullptr; int* nw = nullptr;        // [max_frames][cap], [max_frames][cap], [max_frames]
  float* feat = nullptr; int* n = nullptr;                                   // keep_features: [max_frames][cap][259], [max_frames]
  DevBlock q_scratch;                                                        // query: dense sharing + score [Q][N]
  DevBlock m_scratch;                                                        // composite: the pair batch
  // map state (airfe_bowdb_attach_map): per-frame map points, the covisibility graph in CSR form, keyframe positions
  int has_map = 0, max_edges = 0, has_pos = 0;
  DevBlock map_tables;                                                       // attach_map: xyz, the graph, pos, pose, u_right
  double* xyz = nullptr;                                                     // [max_frames][cap][3], NaN = no valid map point at this feature row
  int32_t *cov_row = nullptr, *cov_nbr = nullptr, *cov_weight = nullptr;     // [max_frames + 1], [max_edges], [max_edges]
  double* pos = nullptr;                                                     // [max_frames][3]
  DevBlock r_scratch;                                                        // relocalisation composite: everything between its kernels
  // loop detection (airfe_bowdb_set_poses / set_u_right): the keyframes' Twc and the right-image columns of their feature rows
  int has_pose = 0;
  double* pose = nullptr;                                                    // [max_frames][16], identity until set
  double* u_right = nullptr;                                                 // [max_frames][cap], -1 until set (> 0: stereo)
  DevBlock l_scratch;                                                        // stored queries / loop detection composite
  // map-point ids (airfe_bowdb_attach_point_ids): what the covisibility build reads
  int max_points = 0;
  DevBlock id_table;                                                         // attach_point_ids: point_id
  int32_t* point_id = nullptr;                                               // [max_frames][cap], -1 = no valid map point at this feature row
  DevBlock c_scratch;                                                        // covisibility build: the per-point and per-row work arrays, sized at attach
  // map-point triangulation (airfe_bowdb_attach_triangulation): the observation segments and the host form's outputs, sized at attach
  int has_tri = 0;
  DevBlock t_scratch;
  // map-point merge (airfe_bowdb_attach_merge): per point the parent, flags, src, best and root, per feature row the adoption staging, sized at attach
  int has_merge = 0;
  DevBlock g_scratch;
  DevBlock g_pairs;                                                          // airfe_bowdb_merge_points: the host pair list's device copy (grows with P)
  // junction state (airfe_bowdb_attach_junctions): per stored frame its words and the two tables of junction_core.h; the same for max_queries queries
  struct JunctionTables {
    unsigned *uword = nullptr; int *wcnt = nullptr, *wconn = nullptr, *nuw = nullptr;          // [rows][cap] x 3, [rows]
    unsigned long long* ukey = nullptr; int *kcnt = nullptr, *nuk = nullptr, *status = nullptr;  // [rows][ecap] x 2, [rows] x 2
  };
  int j_ecap = 0, j_maxq = 0;
  DevBlock j_block;                                                          // everything below, reserved once at attach
  unsigned* j_word = nullptr; int* j_nj = nullptr;                           // [max_frames][cap], [max_frames]
  JunctionTables j_frames, j_queries;
  double* j_score = nullptr; int* j_sharing = nullptr;                       // [max_queries][max_frames]: bowdb_query_kernel's dense outputs
  unsigned *j_ids = nullptr, *j_qword = nullptr; double* j_vals = nullptr;   // the composites' chain for max_queries frames: the vector ...
  int *j_nw = nullptr, *j_qnj = nullptr, *j_nedge = nullptr, *j_qstatus = nullptr; int32_t* j_edge = nullptr;      // ... and the connections
};

// how every entry that takes a database starts: a null database is an error return, and the database's context makes its device current (AIRFE_ENTER)
#define BOWDB_ENTER(db) do { if (!(db)) return 1; AIRFE_ENTER((db)->c); } while (0)

// An attach stage's freshly reserved block goes back unless the stage reaches keep(), where it sets its pointers and flag: a failed attach leaves the database as it
// was, and a later one may succeed.
struct AttachGuard { airfe_ctx* c; DevBlock* b; ~AttachGuard() { if (b) release(c, *b); } void keep() { b = nullptr; } };

// rows first_frame .. first_frame + B - 1 of a [max_frames][per] table, to the table (src) or from it (dst); `table` is null until its stage is attached, and
// `missing` names that stage.  Device to device: asynchronous on st; otherwise synchronous.
template <class T>
int table_rows_copy(airfe_bowdb* db, T* table, const char* missing, size_t per, int first_frame, int B, const void* src, void* dst, hipMemcpyKind kind,
                    hipStream_t st, const char* who) {
  airfe_ctx* c = db->c;
  if (!table) return fail(c, std::string(who) + ": no " + missing);
  if (first_frame < 0 || B < 1 || B > db->max_frames - first_frame || (!src && !dst)) return fail(c, std::string(who) + ": bad argument (frames beyond max_frames)");
  T* at = table + (size_t)first_frame * per;
  if (src) HIPCHK(c, hipMemcpyAsync(at, src, (size_t)B * per * sizeof(T), kind, st));
  else HIPCHK(c, hipMemcpyAsync(dst, at, (size_t)B * per * sizeof(T), kind, st));
  if (kind != hipMemcpyDeviceToDevice) HIPCHK(c, hipStreamSynchronize(st));
  return 0;
}

// ---- airfe_bowdb.hip: queued by its own entries and by the junction composites of airfe_junction.hip
int bow_vector_queue(airfe_ctx* c, const float* d_feat, const int* d_n, int B, int cap, uint32_t* d_ids, double* d_vals, int* d_nw, uint32_t* d_word, hipStream_t st);
int bowdb_add_impl(airfe_bowdb* db, const uint32_t* ids, const double* vals, const int* nw, const float* feat, const int* n, int B, int cap, hipMemcpyKind kind,
                   hipStream_t st, const char* who);
// bowdb_query_kernel over the whole database for Q vectors of qcap rows: the one statement of its arguments and of how the frames are sliced (which changes no
// result).  -> the dense [Q][N] score / sharing; returns the frames per workgroup in *frames_per_wg when asked; the LDS refusal is reported under `who`.
int bowdb_dense_query_queue(airfe_bowdb* db, const uint32_t* d_ids, const double* d_vals, const int* d_nw, int Q, int qcap, double* d_score, int32_t* d_sharing,
                            int* frames_per_wg, hipStream_t st, const char* who);
