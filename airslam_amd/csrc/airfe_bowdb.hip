// airfe — the BoW side of libairfe.so (include/airfe.h): the BoW vector, the device-resident keyframe database with its queries, the grouping, and the
// relocalisation and loop detection composites, the covisibility build and the map-point triangulation (kernels_bowdb.hip, kernels_bowgroup.hip, kernels_loopdet.hip, kernels_covis.hip,
// kernels_triangulate.hip).  The vocabulary itself (airfe_bow_load,
// airfe_bow_transform*) is loaded in airfe.hip.
#include "airfe_host.h"
#include "fransac_core.h"
#include "pnp_core.h"
#include "poseopt_core.h"
#include "bowgroup_core.h"
#include "loopdet_core.h"
#include "covis_core.h"
#include "triangulate_core.h"
#include "junction_core.h"

/* ---- BoW keyframe database (include/airfe.h "BoW keyframe database"; kernels_bowdb.hip): the database object is a C++ struct behind an opaque pointer */
struct airfe_bowdb {
  airfe_ctx* c = nullptr;
  int max_frames = 0, cap = 0, keep = 0, size = 0;
  uint32_t* ids = nullptr; double* vals = nullptr; int* nw = nullptr;        // [max_frames][cap], [max_frames][cap], [max_frames]
  float* feat = nullptr; int* n = nullptr;                                   // keep_features: [max_frames][cap][259], [max_frames]
  DevBlock q_scratch;                                                        // query: dense sharing + score [Q][N]
  DevBlock m_scratch;                                                        // composite: the pair batch
  // map state (airfe_bowdb_attach_map): per-frame map points, the covisibility graph in CSR form, keyframe positions
  int has_map = 0, max_edges = 0, has_pos = 0;
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
  int32_t* point_id = nullptr;                                               // [max_frames][cap], -1 = no valid map point at this feature row
  DevBlock c_scratch;                                                        // covisibility build: the per-point and per-row work arrays, sized at attach
  // map-point triangulation (airfe_bowdb_attach_triangulation): the observation segments and the host form's outputs, sized at attach
  int has_tri = 0;
  DevBlock t_scratch;
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

namespace {
int bow_vector_queue(airfe_ctx* c, const float* d_feat, const int* d_n, int B, int cap, uint32_t* d_ids, double* d_vals, int* d_nw, uint32_t* d_word,
                     hipStream_t st) {
  const size_t rows = (size_t)B * cap;
  Carve k;
  const size_t o_word = k.take(rows * 4), o_wf = k.take(rows * 4), o_node = k.take(rows * 4);
  if (k.into(c, c->bv_scratch, st)) return 1;
  unsigned* word = d_word ? d_word : k.at<unsigned>(o_word);
  float* wf = k.at<float>(o_wf);
  int* node = k.i(o_node);
  ProfScope ps(c, ST_BOW, st, 0, (double)rows * 259 * 4);
  // the existing descent over every row of the batch (rows past a frame's count are descended too and ignored: the vector kernel reads n rows)
  launch_bow_transform(d_feat, AIRFE_FEAT_DIM, 3, (int)rows, c->bow_desc, c->bow_first, c->bow_nch, c->bow_word, c->bow_weight, word, wf, node, st);
  BowVecArgs a;
  a.word = word; a.node = node; a.n = d_n; a.cap = cap; a.weight = c->bow_weight_d; a.ids = d_ids; a.vals = d_vals; a.nw = d_nw;
  launch_bow_vector(a, B, st);
  note_launch(c, ST_BOW);
  HIPCHK(c, hipGetLastError());
  return 0;
}
}  // namespace

extern "C" {

int airfe_bow_vector_batch_dev(airfe_ctx* c, const float* d_feat, const int* d_n, int B, int cap, uint32_t* d_ids, double* d_vals, int* d_nw,
                               uint32_t* d_word, void* stream) try {
  AIRFE_ENTER(c);
  if (!c->bow_nodes) return fail(c, "bow_vector_batch_dev: no vocabulary loaded (airfe_bow_load)");
  if (B < 1 || cap < 1 || !d_feat || !d_n || !d_ids || !d_vals || !d_nw) return fail(c, "bow_vector_batch_dev: bad argument");
  if (cap > BOW_MAX_FEATURES) return fail(c, "bow_vector_batch_dev: cap > 1024");
  if ((size_t)B * cap > (size_t)INT32_MAX) return fail(c, "bow_vector_batch_dev: batch too large");
  return bow_vector_queue(c, d_feat, d_n, B, cap, d_ids, d_vals, d_nw, d_word, stream ? (hipStream_t)stream : c->stream);
} AIRFE_CATCH(c)

int airfe_bow_vector(airfe_ctx* c, const float* feat, int n, uint32_t* ids, double* vals, int* nw, uint32_t* word_of_features) try {
  AIRFE_ENTER(c);
  if (!c->bow_nodes) return fail(c, "bow_vector: no vocabulary loaded (airfe_bow_load)");
  if (n < 0 || !nw || (n > 0 && (!feat || !ids || !vals))) return fail(c, "bow_vector: bad argument");
  if (n > BOW_MAX_FEATURES) return fail(c, "bow_vector: more than 1024 features");
  *nw = 0;
  if (n == 0) return 0;                                          // database.cc:60
  hipStream_t st = c->stream;
  Carve kc;
  const size_t o_n = kc.take(4), o_nw = kc.take(4), o_vals = kc.take((size_t)n * 8), o_feat = kc.take((size_t)n * AIRFE_FEAT_DIM * 4), o_ids = kc.take((size_t)n * 4),
               o_word = kc.take((size_t)n * 4);
  if (kc.into(c, c->bv_stage, st)) return 1;
  int *d_n = kc.i(o_n), *d_nw = kc.i(o_nw);
  double* d_vals = kc.d(o_vals);
  float* d_feat = kc.at<float>(o_feat);
  uint32_t *d_ids = kc.at<uint32_t>(o_ids), *d_word = kc.at<uint32_t>(o_word);
  DrainOnError drain{c, true};
  HIPCHK(c, hipMemcpyAsync(d_n, &n, 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_feat, feat, (size_t)n * AIRFE_FEAT_DIM * 4, hipMemcpyHostToDevice, st));
  if (bow_vector_queue(c, d_feat, d_n, 1, n, d_ids, d_vals, d_nw, d_word, st)) return 1;
  int k = 0;
  HIPCHK(c, hipMemcpyAsync(&k, d_nw, 4, hipMemcpyDeviceToHost, st));
  if (word_of_features) HIPCHK(c, hipMemcpyAsync(word_of_features, d_word, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (k > 0) {
    HIPCHK(c, hipMemcpyAsync(ids, d_ids, (size_t)k * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(vals, d_vals, (size_t)k * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
  }
  drain.armed = false;
  *nw = k;
  return 0;
} AIRFE_CATCH(c)

int airfe_bowdb_create(airfe_ctx* c, int max_frames, int cap, int keep_features, airfe_bowdb** out) try {
  AIRFE_ENTER(c);
  if (!out) return fail(c, "bowdb_create: null argument");
  *out = nullptr;
  if (max_frames < 1 || cap < 1) return fail(c, "bowdb_create: bad argument");
  if (cap > BOW_MAX_FEATURES) return fail(c, "bowdb_create: cap > 1024");
  if (!c->bow_nodes) return fail(c, "bowdb_create: no vocabulary loaded (airfe_bow_load): the database is sized by its word count");
  struct Guard { airfe_bowdb* p; ~Guard() { if (p) (void)airfe_bowdb_destroy(p); } } guard{new airfe_bowdb()};
  airfe_bowdb* db = guard.p;
  db->c = c; db->max_frames = max_frames; db->cap = cap; db->keep = keep_features != 0;
  const size_t rows = (size_t)max_frames * cap;
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&db->ids), rows * 4));
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&db->vals), rows * 8));
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&db->nw), (size_t)max_frames * 4));
  if (db->keep) {
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&db->feat), rows * AIRFE_FEAT_DIM * 4));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&db->n), (size_t)max_frames * 4));
  }
  guard.p = nullptr;
  *out = db;
  return 0;
} AIRFE_CATCH(c)

int airfe_bowdb_destroy(airfe_bowdb* db) try {
  if (!db) return 0;
  if (db->c) { (void)enter_device(db->c); (void)hipDeviceSynchronize(); }
  for (void* p : {(void*)db->ids, (void*)db->vals, (void*)db->nw, (void*)db->feat, (void*)db->n, (void*)db->xyz, (void*)db->cov_row, (void*)db->cov_nbr,
                  (void*)db->cov_weight, (void*)db->pos, (void*)db->pose, (void*)db->u_right, (void*)db->point_id})      // the persistent tables
    if (p) (void)hipFree(p);
  if (db->c)
    for (DevBlock* b : {&db->q_scratch, &db->m_scratch, &db->r_scratch, &db->l_scratch, &db->c_scratch, &db->t_scratch, &db->j_block}) release(db->c, *b);
  delete db;
  return 0;
} AIRFE_CATCH(nullptr)

int airfe_bowdb_clear(airfe_bowdb* db) try {
  if (!db) return 1;
  db->size = 0;
  return 0;
} AIRFE_CATCH(db->c)

int airfe_bowdb_size(const airfe_bowdb* db) try {
  return db ? db->size : -1;
} AIRFE_CATCH(nullptr)

// Database::AddFrame: frame `size + b` = vector b.  kind = hipMemcpyDeviceToDevice (asynchronous on st) or hipMemcpyHostToDevice (synchronous)
static int bowdb_add_impl(airfe_bowdb* db, const uint32_t* ids, const double* vals, const int* nw, const float* feat, const int* n, int B, int cap,
                          hipMemcpyKind kind, hipStream_t st, const char* who) {
  airfe_ctx* c = db->c;
  if (B < 1 || !ids || !vals || !nw || cap != db->cap) return fail(c, std::string(who) + ": bad argument (cap must be the database's)");
  if (db->keep && (!feat || !n)) return fail(c, std::string(who) + ": this database keeps the frames' features: d_feat / d_n are needed");
  if (B > db->max_frames - db->size) return fail(c, std::string(who) + ": the database is full (max_frames)");
  const size_t at = (size_t)db->size * cap, rows = (size_t)B * cap;
  HIPCHK(c, hipMemcpyAsync(db->ids + at, ids, rows * 4, kind, st));
  HIPCHK(c, hipMemcpyAsync(db->vals + at, vals, rows * 8, kind, st));
  HIPCHK(c, hipMemcpyAsync(db->nw + db->size, nw, (size_t)B * 4, kind, st));
  if (db->keep) {
    HIPCHK(c, hipMemcpyAsync(db->feat + at * AIRFE_FEAT_DIM, feat, rows * AIRFE_FEAT_DIM * 4, kind, st));
    HIPCHK(c, hipMemcpyAsync(db->n + db->size, n, (size_t)B * 4, kind, st));
  }
  if (kind == hipMemcpyHostToDevice) HIPCHK(c, hipStreamSynchronize(st));
  db->size += B;
  return 0;
}

int airfe_bowdb_add_batch_dev(airfe_bowdb* db, const uint32_t* d_ids, const double* d_vals, const int* d_nw, const float* d_feat, const int* d_n, int B,
                              int cap, void* stream) try {
  if (!db) return 1;
  AIRFE_ENTER(db->c);
  return bowdb_add_impl(db, d_ids, d_vals, d_nw, d_feat, d_n, B, cap, hipMemcpyDeviceToDevice, stream ? (hipStream_t)stream : db->c->stream, "bowdb_add_batch_dev");
} AIRFE_CATCH(db->c)

int airfe_bowdb_add(airfe_bowdb* db, const uint32_t* ids, const double* vals, const int* nw, const float* feat, const int* n, int B, int cap) try {
  if (!db) return 1;
  AIRFE_ENTER(db->c);
  return bowdb_add_impl(db, ids, vals, nw, feat, n, B, cap, hipMemcpyHostToDevice, db->c->stream, "bowdb_add");
} AIRFE_CATCH(db->c)

// Database::Query + the sharing-word filter + Database::Score for Q device vectors on `st` (the body of airfe_bowdb_query_batch_dev; the relocalisation
// composite queues the same code)
static int bowdb_query_queue(airfe_bowdb* db, const uint32_t* d_ids, const double* d_vals, const int* d_nw, int Q, int cap, const airfe_bowdb_filter* filter,
                             int32_t* d_cand_frame, int32_t* d_cand_sharing, double* d_cand_score, int ccap, int* d_ncand, int* d_max_sharing,
                             int32_t* d_sharing, hipStream_t st) {
  airfe_ctx* c = db->c;
  const int N = db->size;
  const size_t cells = (size_t)Q * std::max(N, 1);
  Carve k;
  const size_t o_score = k.take(cells * 8), o_sharing = k.take(cells * 4);
  if (k.into(c, db->q_scratch, st)) return 1;
  BowQueryArgs a;
  a.db_ids = db->ids; a.db_vals = db->vals; a.db_nw = db->nw; a.N = N; a.cap = db->cap;
  a.q_ids = d_ids; a.q_vals = d_vals; a.q_nw = d_nw; a.qcap = cap; a.n_words = c->bow_nwords;
  a.frames_per_wg = (size_t)Q * N >= (size_t)64 * 1024 ? 64 : 16;     // (how the frames are sliced changes no result)
  a.score = k.d(o_score);
  a.sharing = d_sharing ? d_sharing : k.i(o_sharing);
  ProfScope ps(c, ST_BOW, st, 0, (double)Q * N * db->cap * 12);
  if (launch_bowdb_query(a, Q, st)) return fail(c, "bowdb_query_batch_dev: the query table does not fit the workgroup's LDS");
  BowSelectArgs s;
  s.sharing = a.sharing; s.score = a.score; s.N = N; s.ratio = filter->ratio; s.min_words = filter->min_words;
  s.max_index = filter->d_max_index; s.exclude = filter->d_exclude; s.exclude_words = filter->exclude_words;
  s.cand_frame = d_cand_frame; s.cand_sharing = d_cand_sharing; s.cand_score = d_cand_score; s.ccap = ccap; s.ncand = d_ncand; s.max_sharing = d_max_sharing;
  launch_bowdb_select(s, Q, st);
  note_launch(c, ST_BOW);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int airfe_bowdb_query_batch_dev(airfe_bowdb* db, const uint32_t* d_ids, const double* d_vals, const int* d_nw, int Q, int cap,
                                const airfe_bowdb_filter* filter, int32_t* d_cand_frame, int32_t* d_cand_sharing, double* d_cand_score, int ccap,
                                int* d_ncand, int* d_max_sharing, int32_t* d_sharing, void* stream) try {
  if (!db) return 1;
  airfe_ctx* c = db->c;
  AIRFE_ENTER(c);
  if (Q < 1 || cap < 1 || ccap < 1 || !d_ids || !d_vals || !d_nw || !filter || !d_cand_frame || !d_cand_sharing || !d_cand_score || !d_ncand || !d_max_sharing)
    return fail(c, "bowdb_query_batch_dev: bad argument");
  if (cap > BOW_MAX_FEATURES) return fail(c, "bowdb_query_batch_dev: cap > 1024");
  if (filter->d_exclude && filter->exclude_words < 1) return fail(c, "bowdb_query_batch_dev: d_exclude needs exclude_words");
  return bowdb_query_queue(db, d_ids, d_vals, d_nw, Q, cap, filter, d_cand_frame, d_cand_sharing, d_cand_score, ccap, d_ncand, d_max_sharing, d_sharing,
                           stream ? (hipStream_t)stream : c->stream);
} AIRFE_CATCH(db->c)

int airfe_bowdb_topk_dev(airfe_bowdb* db, const int32_t* d_cand_frame, const double* d_cand_score, const int* d_ncand, int Q, int ccap, int K,
                         int32_t* d_top, double* d_top_score, void* stream) try {
  if (!db) return 1;
  airfe_ctx* c = db->c;
  AIRFE_ENTER(c);
  if (Q < 1 || ccap < 1 || K < 1 || K > 8 || !d_cand_frame || !d_cand_score || !d_ncand || !d_top) return fail(c, "bowdb_topk_dev: bad argument (K = 1..8)");
  BowTopkArgs a;
  a.cand_frame = d_cand_frame; a.cand_score = d_cand_score; a.ncand = d_ncand; a.ccap = ccap; a.K = K; a.top = d_top; a.top_score = d_top_score;
  launch_bowdb_topk(a, Q, stream ? (hipStream_t)stream : c->stream);
  HIPCHK(c, hipGetLastError());
  return 0;
} AIRFE_CATCH(db->c)

// the best-candidate rule around the matcher for Q queries x K candidates on `st` (the body of airfe_bowdb_match_candidates_batch_dev; the relocalisation
// composite queues the same code)
static int bowdb_match_queue(airfe_ctx* c, airfe_bowdb* db, const float* d_qfeat, const int* d_qn, int Q, int cap, const int32_t* d_cand, int K,
                             int outlier_rejection, int32_t* d_best, int32_t* d_idx, float* d_score, int mcap, int* d_nmatch, int* d_nmatch_all,
                             hipStream_t st) {
  const int P = Q * K;
  Carve k;
  const size_t fb = (size_t)P * cap * AIRFE_FEAT_DIM * 4, cb = (size_t)P * 4;
  const size_t o_f0 = k.take(fb), o_f1 = k.take(fb), o_idx = k.take((size_t)P * mcap * 8), o_score = k.take((size_t)P * mcap * 4), o_n0 = k.take(cb),
               o_n1 = k.take(cb), o_nm = k.take(cb);
  if (k.into(c, db->m_scratch, st)) return 1;
  BowGatherArgs g;
  g.f0 = k.at<float>(o_f0); g.f1 = k.at<float>(o_f1); g.n0 = k.i(o_n0); g.n1 = k.i(o_n1);
  int32_t* p_idx = k.at<int32_t>(o_idx);
  float* p_score = k.at<float>(o_score);
  int* p_nm = k.i(o_nm);
  g.qfeat = d_qfeat; g.qn = d_qn; g.db_feat = db->feat; g.db_n = db->n; g.N = db->size; g.cap = cap; g.cand = d_cand; g.K = K;
  launch_bowdb_gather(g, P, st);
  HIPCHK(c, hipGetLastError());
  // MatchingPoints(query_features, good_candidate_features, matches, true) (map_user.cc:369): the context's own entries, called
  if (lightglue_dev(c, g.f0, g.n0, g.f1, g.n1, P, cap, AIRFE_FEAT_DIM, 1, 1, p_idx, p_score, mcap, p_nm, nullptr, st)) return 1;
  if (outlier_rejection && fransac_queue(c, g.f0, g.f1, P, cap, p_idx, p_score, mcap, p_nm, nullptr, st)) return 1;
  BowBestArgs b;
  b.cand = d_cand; b.K = K; b.N = db->size; b.mcap = mcap; b.idx_all = p_idx; b.score_all = p_score; b.nmatch_all = p_nm;
  b.best = d_best; b.idx = d_idx; b.score = d_score; b.nmatch = d_nmatch; b.out_nmatch_all = d_nmatch_all;
  launch_bowdb_best(b, Q, st);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int airfe_bowdb_match_candidates_batch_dev(airfe_ctx* c, airfe_bowdb* db, const float* d_qfeat, const int* d_qn, int Q, int cap, const int32_t* d_cand, int K,
                                           int outlier_rejection, int32_t* d_best, int32_t* d_idx, float* d_score, int mcap, int* d_nmatch,
                                           int* d_nmatch_all, void* stream) try {
  AIRFE_ENTER(c);
  if (!db || db->c != c) return fail(c, "bowdb_match_candidates_batch_dev: the database belongs to another context");
  if (Q < 1 || K < 1 || K > 5 || mcap < 1 || !d_qfeat || !d_qn || !d_cand || !d_best || !d_idx || !d_score || !d_nmatch)
    return fail(c, "bowdb_match_candidates_batch_dev: bad argument (K = 1..5)");
  if (!db->keep) return fail(c, "bowdb_match_candidates_batch_dev: the database was created without keep_features");
  if (cap != db->cap) return fail(c, "bowdb_match_candidates_batch_dev: cap must be the database's");
  if (mcap > FR_MAX_MATCHES) return fail(c, "bowdb_match_candidates_batch_dev: mcap > 1024");
  if ((long long)Q * K > c->Pmax) return fail(c, "bowdb_match_candidates_batch_dev: Q * K pairs exceed cfg.max_batch");
  return bowdb_match_queue(c, db, d_qfeat, d_qn, Q, cap, d_cand, K, outlier_rejection, d_best, d_idx, d_score, mcap, d_nmatch, d_nmatch_all,
                           stream ? (hipStream_t)stream : c->stream);
} AIRFE_CATCH(c)

/* ---- map state in the database, the grouping and the relocalisation composite (include/airfe.h "Grouping", "Relocalisation composite";
 * kernels_bowgroup.hip, bowgroup_core.h) ------------------------------------------------------------------------------------------------------------ */
int airfe_bowdb_attach_map(airfe_bowdb* db, int max_edges) try {
  if (!db) return 1;
  airfe_ctx* c = db->c;
  AIRFE_ENTER(c);
  if (db->has_map) return fail(c, "bowdb_attach_map: the map state is attached already");
  if (!db->keep) return fail(c, "bowdb_attach_map: the database was created without keep_features");
  if (max_edges < 1) return fail(c, "bowdb_attach_map: bad argument");
  const size_t rows = (size_t)db->max_frames * db->cap;
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&db->xyz), rows * 24));
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&db->cov_row), ((size_t)db->max_frames + 1) * 4));
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&db->cov_nbr), (size_t)max_edges * 4));
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&db->cov_weight), (size_t)max_edges * 4));
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&db->pos), (size_t)db->max_frames * 24));
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&db->pose), (size_t)db->max_frames * 128));
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&db->u_right), rows * 8));
  HIPCHK(c, hipMemsetAsync(db->xyz, 0xFF, rows * 24, c->stream));                         // every byte 0xFF: a NaN in every slot
  HIPCHK(c, hipMemsetAsync(db->cov_row, 0, ((size_t)db->max_frames + 1) * 4, c->stream));  // an empty graph
  HIPCHK(c, hipMemsetAsync(db->cov_nbr, 0, (size_t)max_edges * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(db->cov_weight, 0, (size_t)max_edges * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(db->pos, 0xFF, (size_t)db->max_frames * 24, c->stream));
  launch_loopdet_init(db->pose, db->u_right, db->max_frames, db->cap, c->stream);          // identity poses, no right image anywhere
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  db->max_edges = max_edges;
  db->has_map = 1;
  return 0;
} AIRFE_CATCH(db->c)

// rows first_frame .. first_frame + B - 1 of a [max_frames][per] f64 table
static int bowdb_rows_copy(airfe_bowdb* db, double* table, size_t per, int first_frame, int B, const void* src, void* dst, hipMemcpyKind kind, hipStream_t st,
                           const char* who) {
  airfe_ctx* c = db->c;
  if (!db->has_map) return fail(c, std::string(who) + ": no map state (airfe_bowdb_attach_map)");
  if (first_frame < 0 || B < 1 || B > db->max_frames - first_frame || (!src && !dst)) return fail(c, std::string(who) + ": bad argument (frames beyond max_frames)");
  double* at = table + (size_t)first_frame * per;
  if (src) HIPCHK(c, hipMemcpyAsync(at, src, (size_t)B * per * 8, kind, st));
  else HIPCHK(c, hipMemcpyAsync(dst, at, (size_t)B * per * 8, kind, st));
  if (kind != hipMemcpyDeviceToDevice) HIPCHK(c, hipStreamSynchronize(st));
  return 0;
}

int airfe_bowdb_set_points_dev(airfe_bowdb* db, int first_frame, int B, const double* d_xyz, void* stream) try {
  if (!db) return 1;
  AIRFE_ENTER(db->c);
  return bowdb_rows_copy(db, db->xyz, (size_t)db->cap * 3, first_frame, B, d_xyz, nullptr, hipMemcpyDeviceToDevice,
                         stream ? (hipStream_t)stream : db->c->stream, "bowdb_set_points_dev");
} AIRFE_CATCH(db->c)

int airfe_bowdb_set_points(airfe_bowdb* db, int first_frame, int B, const double* xyz) try {
  if (!db) return 1;
  AIRFE_ENTER(db->c);
  return bowdb_rows_copy(db, db->xyz, (size_t)db->cap * 3, first_frame, B, xyz, nullptr, hipMemcpyHostToDevice, db->c->stream, "bowdb_set_points");
} AIRFE_CATCH(db->c)

int airfe_bowdb_get_points(airfe_bowdb* db, int first_frame, int B, double* xyz) try {
  if (!db) return 1;
  AIRFE_ENTER(db->c);
  return bowdb_rows_copy(db, db->xyz, (size_t)db->cap * 3, first_frame, B, nullptr, xyz, hipMemcpyDeviceToHost, db->c->stream, "bowdb_get_points");
} AIRFE_CATCH(db->c)

int airfe_bowdb_set_positions(airfe_bowdb* db, int first_frame, int B, const double* pos) try {
  if (!db) return 1;
  AIRFE_ENTER(db->c);
  if (bowdb_rows_copy(db, db->pos, 3, first_frame, B, pos, nullptr, hipMemcpyHostToDevice, db->c->stream, "bowdb_set_positions")) return 1;
  db->has_pos = 1;
  return 0;
} AIRFE_CATCH(db->c)

int airfe_bowdb_set_covisibility(airfe_bowdb* db, const int32_t* row_ptr, const int32_t* nbr, const int32_t* weight, int n_frames) try {
  if (!db) return 1;
  airfe_ctx* c = db->c;
  AIRFE_ENTER(c);
  if (!db->has_map) return fail(c, "bowdb_set_covisibility: no map state (airfe_bowdb_attach_map)");
  if (n_frames < 0 || n_frames > db->max_frames || !row_ptr) return fail(c, "bowdb_set_covisibility: bad argument (n_frames beyond max_frames)");
  if (row_ptr[0] != 0) return fail(c, "bowdb_set_covisibility: row_ptr[0] must be 0");
  for (int f = 0; f < n_frames; ++f)
    if (row_ptr[f + 1] < row_ptr[f]) return fail(c, "bowdb_set_covisibility: row_ptr must not decrease");
  const int E = row_ptr[n_frames];
  if (E > db->max_edges) return fail(c, "bowdb_set_covisibility: more entries than max_edges");
  if (E > 0 && (!nbr || !weight)) return fail(c, "bowdb_set_covisibility: bad argument");
  for (int f = 0; f < n_frames; ++f)
    for (int e = row_ptr[f]; e < row_ptr[f + 1]; ++e)
      if (nbr[e] < 0 || (e > row_ptr[f] && nbr[e] <= nbr[e - 1]))
        return fail(c, "bowdb_set_covisibility: every row must be strictly ascending in nbr (nothing was changed)");
  std::vector<int32_t> rows((size_t)db->max_frames + 1, E);                                // frames past n_frames: empty rows
  std::copy(row_ptr, row_ptr + n_frames + 1, rows.begin());
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemcpyAsync(db->cov_row, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, st));
  if (E > 0) {
    HIPCHK(c, hipMemcpyAsync(db->cov_nbr, nbr, (size_t)E * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(db->cov_weight, weight, (size_t)E * 4, hipMemcpyHostToDevice, st));
  }
  HIPCHK(c, hipStreamSynchronize(st));
  return 0;
} AIRFE_CATCH(db->c)

int airfe_bowdb_get_covisibility(airfe_bowdb* db, int32_t* row_ptr, int32_t* nbr, int32_t* weight, int edge_cap, int* n_edges) try {
  if (!db) return 1;
  airfe_ctx* c = db->c;
  AIRFE_ENTER(c);
  if (!db->has_map) return fail(c, "bowdb_get_covisibility: no map state (airfe_bowdb_attach_map)");
  if (!row_ptr || !n_edges || edge_cap < 0) return fail(c, "bowdb_get_covisibility: bad argument");
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemcpyAsync(row_ptr, db->cov_row, ((size_t)db->max_frames + 1) * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  const int E = row_ptr[db->max_frames];
  *n_edges = E;
  if (E > edge_cap) return fail(c, "bowdb_get_covisibility: more entries than edge_cap");
  if (E > 0) {
    if (!nbr || !weight) return fail(c, "bowdb_get_covisibility: bad argument");
    HIPCHK(c, hipMemcpyAsync(nbr, db->cov_nbr, (size_t)E * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(weight, db->cov_weight, (size_t)E * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
  }
  return 0;
} AIRFE_CATCH(db->c)

// the grouping for Q candidate lists on `st`
static int bowdb_group_queue(airfe_bowdb* db, int mode, const int32_t* d_cand_frame, const double* d_cand_score, const int* d_ncand, int Q, int ccap, int K,
                             const double* d_extra, const double* d_qpos, const double* d_max_dist, int32_t* d_group_frame, double* d_group_score,
                             int* d_ngroups, int* d_status, hipStream_t st) {
  airfe_ctx* c = db->c;
  BowGroupArgs a;
  a.mode = mode; a.cand_frame = d_cand_frame; a.cand_score = d_cand_score; a.ncand = d_ncand; a.ccap = ccap; a.K = K;
  a.row_ptr = db->cov_row; a.nbr = db->cov_nbr; a.weight = db->cov_weight; a.rows = db->max_frames;
  a.extra = d_extra; a.n_extra = db->size; a.pos = db->pos; a.pos_rows = db->max_frames; a.qpos = d_qpos; a.max_dist = d_max_dist;
  a.group_frame = d_group_frame; a.group_score = d_group_score; a.ngroups = d_ngroups; a.status = d_status;
  if (launch_bowgroup(a, Q, st)) return fail(c, "bowdb_group_dev: the candidate list does not fit the workgroup's LDS");
  HIPCHK(c, hipGetLastError());
  return 0;
}

int airfe_bowdb_group_dev(airfe_bowdb* db, int mode, const int32_t* d_cand_frame, const double* d_cand_score, const int* d_ncand, int Q, int ccap, int K,
                          const double* d_extra, const double* d_qpos, const double* d_max_dist, int32_t* d_group_frame, double* d_group_score,
                          int* d_ngroups, int* d_status, void* stream) try {
  if (!db) return 1;
  airfe_ctx* c = db->c;
  AIRFE_ENTER(c);
  if (!db->has_map) return fail(c, "bowdb_group_dev: no map state (airfe_bowdb_attach_map)");
  if (Q < 1 || ccap < 1 || K < 1 || !d_cand_frame || !d_cand_score || !d_ncand || !d_group_frame || !d_group_score || !d_ngroups || !d_status)
    return fail(c, "bowdb_group_dev: bad argument");
  if (mode != BG_MODE_RELOC && mode != BG_MODE_LOOP) return fail(c, "bowdb_group_dev: mode is 0 (relocalisation) or 1 (loop detection)");
  if (K > (mode == BG_MODE_RELOC ? 3 : 5)) return fail(c, "bowdb_group_dev: K <= 3 (relocalisation) / K <= 5 (loop detection)");
  if (ccap > BG_MAX_CAND) return fail(c, "bowdb_group_dev: ccap > 4096");
  if (mode == BG_MODE_LOOP && (!d_qpos || !d_max_dist || !db->has_pos))
    return fail(c, "bowdb_group_dev: the loop form needs d_qpos, d_max_dist and the keyframe positions (airfe_bowdb_set_positions)");
  return bowdb_group_queue(db, mode, d_cand_frame, d_cand_score, d_ncand, Q, ccap, K, d_extra, d_qpos, d_max_dist, d_group_frame, d_group_score, d_ngroups,
                           d_status, stream ? (hipStream_t)stream : c->stream);
} AIRFE_CATCH(db->c)

int airfe_relocalize_batch_dev(airfe_ctx* c, airfe_bowdb* db, const airfe_reloc_cfg* cfg, const float* d_qfeat, const int* d_qn, int Q, int cap,
                               const double* d_extra, int* d_ok, int* d_stage, double* d_Twc, int32_t* d_best, int* d_num, uint8_t* d_mask, int32_t* d_idx,
                               float* d_score, int mcap, int* d_nmatch, int* d_pnp_count, void* stream) try {
  AIRFE_ENTER(c);
  if (!db || db->c != c) return fail(c, "relocalize_batch_dev: the database belongs to another context");
  if (!db->has_map) return fail(c, "relocalize_batch_dev: no map state (airfe_bowdb_attach_map)");
  if (!cfg || Q < 1 || mcap < 1 || !d_qfeat || !d_qn || !d_ok || !d_stage || !d_Twc || !d_best || !d_num || !d_mask || !d_idx || !d_score || !d_nmatch)
    return fail(c, "relocalize_batch_dev: bad argument");
  if (cfg->K < 1 || cfg->K > 3) return fail(c, "relocalize_batch_dev: cfg.K = 1..3");
  if (cap != db->cap) return fail(c, "relocalize_batch_dev: cap must be the database's");
  if (mcap > PNP_MAX_POINTS) return fail(c, "relocalize_batch_dev: mcap > 1024");
  if ((long long)Q * cfg->K > c->Pmax) return fail(c, "relocalize_batch_dev: Q * K pairs exceed cfg.max_batch");
  if (!c->bow_nodes) return fail(c, "relocalize_batch_dev: no vocabulary loaded (airfe_bow_load)");
  const int N = db->size, ccap = std::max(N, 1), K = cfg->K;
  if (ccap > BG_MAX_CAND) return fail(c, "relocalize_batch_dev: more than 4096 frames in the database");
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  // one block, every part 256-byte aligned
  Carve k;
  const size_t qc = (size_t)Q * cap, qm = (size_t)Q * mcap, qcc = (size_t)Q * ccap, qb = (size_t)Q * 4;
  const size_t o_ids = k.take(qc * 4), o_vals = k.take(qc * 8), o_nw = k.take(qb), o_cf = k.take(qcc * 4), o_cs = k.take(qcc * 4), o_sc = k.take(qcc * 8), o_nc = k.take(qb),
               o_ms = k.take(qb), o_gf = k.take((size_t)Q * K * 4), o_gs = k.take((size_t)Q * K * 8), o_ng = k.take(qb), o_gst = k.take(qb), o_obj = k.take(qm * 12),
               o_img = k.take(qm * 8), o_map = k.take(qm * 4), o_X = k.take(qm * 24), o_obs = k.take(qm * 24), o_n = k.take(qb), o_nopt = k.take(qb), o_pre = k.take(qb),
               o_pnp = k.take((size_t)Q * 128), o_pmask = k.take(qm), o_pcnt = k.take(qb);
  if (k.into(c, db->r_scratch, st)) return 1;
  // map_user.cc:129-166: the vector, the query with the sharing-word filter, the scores
  if (bow_vector_queue(c, d_qfeat, d_qn, Q, cap, k.at<uint32_t>(o_ids), k.d(o_vals), k.i(o_nw), nullptr, st)) return 1;
  airfe_bowdb_filter flt;
  flt.ratio = cfg->ratio; flt.min_words = cfg->min_words; flt.d_max_index = nullptr; flt.d_exclude = nullptr; flt.exclude_words = 0;
  if (bowdb_query_queue(db, k.at<uint32_t>(o_ids), k.d(o_vals), k.i(o_nw), Q, cap, &flt, k.i(o_cf), k.i(o_cs), k.d(o_sc), ccap, k.i(o_nc), k.i(o_ms),
                        nullptr, st)) return 1;
  // :177-363: the grouping; :360-376: the matcher over the K deputies
  if (bowdb_group_queue(db, BG_MODE_RELOC, k.i(o_cf), k.d(o_sc), k.i(o_nc), Q, ccap, K, d_extra, nullptr, nullptr, k.i(o_gf), k.d(o_gs), k.i(o_ng), k.i(o_gst), st)) return 1;
  if (bowdb_match_queue(c, db, d_qfeat, d_qn, Q, cap, k.i(o_gf), K, cfg->outlier_rejection, d_best, d_idx, d_score, mcap, d_nmatch, nullptr, st)) return 1;
  // :377-390: the first gate, the winner's map points, SolvePnPWithCV
  const int refine = cfg->pose_refinement != 0;
  RelocGatherArgs g;
  g.xyz = db->xyz; g.N = N; g.cap = cap; g.qfeat = d_qfeat; g.best = d_best; g.idx = d_idx; g.nmatch = d_nmatch; g.mcap = mcap;
  g.ncand = k.i(o_nc); g.gstatus = k.i(o_gst); g.ngroups = k.i(o_ng); g.min_inlier = cfg->min_inlier; g.refine = refine;
  g.obj = k.at<float>(o_obj); g.img = k.at<float>(o_img); g.map = k.i(o_map); g.X = k.d(o_X); g.obs = k.d(o_obs);
  g.n = k.i(o_n); g.n_opt = k.i(o_nopt); g.pre = k.i(o_pre);
  launch_reloc_gather(g, Q, st);
  HIPCHK(c, hipGetLastError());
  RelocFinishArgs f;
  f.pre = g.pre; f.num = d_num; f.min_inlier = cfg->min_inlier; f.stage = d_stage; f.ok = d_ok;
  if (!refine) {
    if (pnp_queue(c, g.obj, g.img, g.n, Q, mcap, cfg->cam, d_Twc, nullptr, d_mask, mcap, g.map, d_num, st)) return 1;
    f.pnp_count = d_num; f.pnp_count_out = d_pnp_count;
  } else {
    // :392-457: the frame optimisation from the PnP pose, Tcb = identity, every constraint mono; fewer constraints than min_inlier: none are handed over
    // and the kernel returns its start pose, PnP's
    int* d_cnt = d_pnp_count ? d_pnp_count : k.i(o_pcnt);
    if (pnp_queue(c, g.obj, g.img, g.n, Q, mcap, cfg->cam, k.d(o_pnp), nullptr, k.at<uint8_t>(o_pmask), mcap, g.map, d_cnt, st)) return 1;
    if (poseopt_queue(c, g.X, g.obs, g.n_opt, Q, mcap, k.d(o_pnp), cfg->cam, nullptr, cfg->thr, d_Twc, nullptr, d_mask, mcap, g.map, d_num, -1, nullptr, st))
      return 1;
  }
  launch_reloc_finish(f, Q, st);
  HIPCHK(c, hipGetLastError());
  return 0;
} AIRFE_CATCH(c)

/* ---- loop detection over a loaded map (include/airfe.h "Map state for loop detection", "Stored queries against their predecessors", "Loop detection
 * composite"; kernels_loopdet.hip, loopdet_core.h) -------------------------------------------------------------------------------------------------- */
int airfe_bowdb_set_poses(airfe_bowdb* db, int first_frame, int B, const double* Twc) try {
  if (!db) return 1;
  airfe_ctx* c = db->c;
  AIRFE_ENTER(c);
  if (!db->has_map) return fail(c, "bowdb_set_poses: no map state (airfe_bowdb_attach_map)");
  if (first_frame < 0 || B < 1 || B > db->max_frames - first_frame || !Twc) return fail(c, "bowdb_set_poses: bad argument (frames beyond max_frames)");
  std::vector<double> t((size_t)B * 3);
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < 3; ++k) t[(size_t)b * 3 + k] = Twc[(size_t)b * 16 + 4 * k + 3];
  if (bowdb_rows_copy(db, db->pose, 16, first_frame, B, Twc, nullptr, hipMemcpyHostToDevice, c->stream, "bowdb_set_poses")) return 1;
  if (bowdb_rows_copy(db, db->pos, 3, first_frame, B, t.data(), nullptr, hipMemcpyHostToDevice, c->stream, "bowdb_set_poses")) return 1;
  db->has_pos = 1;
  db->has_pose = 1;
  return 0;
} AIRFE_CATCH(db->c)

int airfe_bowdb_get_poses(airfe_bowdb* db, int first_frame, int B, double* Twc) try {
  if (!db) return 1;
  AIRFE_ENTER(db->c);
  return bowdb_rows_copy(db, db->pose, 16, first_frame, B, nullptr, Twc, hipMemcpyDeviceToHost, db->c->stream, "bowdb_get_poses");
} AIRFE_CATCH(db->c)

int airfe_bowdb_set_u_right_dev(airfe_bowdb* db, int first_frame, int B, const double* d_u_right, void* stream) try {
  if (!db) return 1;
  AIRFE_ENTER(db->c);
  return bowdb_rows_copy(db, db->u_right, (size_t)db->cap, first_frame, B, d_u_right, nullptr, hipMemcpyDeviceToDevice,
                         stream ? (hipStream_t)stream : db->c->stream, "bowdb_set_u_right_dev");
} AIRFE_CATCH(db->c)

int airfe_bowdb_set_u_right(airfe_bowdb* db, int first_frame, int B, const double* u_right) try {
  if (!db) return 1;
  AIRFE_ENTER(db->c);
  return bowdb_rows_copy(db, db->u_right, (size_t)db->cap, first_frame, B, u_right, nullptr, hipMemcpyHostToDevice, db->c->stream, "bowdb_set_u_right");
} AIRFE_CATCH(db->c)

int airfe_bowdb_get_u_right(airfe_bowdb* db, int first_frame, int B, double* u_right) try {
  if (!db) return 1;
  AIRFE_ENTER(db->c);
  return bowdb_rows_copy(db, db->u_right, (size_t)db->cap, first_frame, B, nullptr, u_right, hipMemcpyDeviceToHost, db->c->stream, "bowdb_get_u_right");
} AIRFE_CATCH(db->c)

// stored frames d_qframe [Q] against their predecessors on `st`: the stored vectors gathered into d_ids / d_vals / d_nw ([Q][cap] x 2, [Q]: the caller's
// scratch), bowdb_query_kernel unchanged over the whole database, the prefix selection (the body of airfe_bowdb_query_stored_batch_dev; the loop
// detection composite queues the same code)
static int loopdet_query_queue(airfe_bowdb* db, const int32_t* d_qframe, int Q, float ratio, int min_words, int exclude_covisible, uint32_t* d_ids,
                               double* d_vals, int* d_nw, int32_t* d_cand_frame, int32_t* d_cand_sharing, double* d_cand_score, int ccap, int* d_ncand,
                               int* d_max_sharing, int32_t* d_sharing, hipStream_t st) {
  airfe_ctx* c = db->c;
  const int N = db->size;
  const size_t cells = (size_t)Q * std::max(N, 1);
  Carve k;
  const size_t o_score = k.take(cells * 8), o_sharing = k.take(cells * 4);
  if (k.into(c, db->q_scratch, st)) return 1;
  LoopQvecArgs v;
  v.qframe = d_qframe; v.db_ids = db->ids; v.db_vals = db->vals; v.db_nw = db->nw; v.N = N; v.cap = db->cap; v.ids = d_ids; v.vals = d_vals; v.nw = d_nw;
  launch_loopdet_qvec(v, Q, st);
  BowQueryArgs a;
  a.db_ids = db->ids; a.db_vals = db->vals; a.db_nw = db->nw; a.N = N; a.cap = db->cap;
  a.q_ids = d_ids; a.q_vals = d_vals; a.q_nw = d_nw; a.qcap = db->cap; a.n_words = c->bow_nwords;
  a.frames_per_wg = (size_t)Q * N >= (size_t)64 * 1024 ? 64 : 16;     // (how the frames are sliced changes no result)
  a.score = k.d(o_score);
  a.sharing = d_sharing ? d_sharing : k.i(o_sharing);
  ProfScope ps(c, ST_BOW, st, 0, (double)Q * N * db->cap * 12);
  if (launch_bowdb_query(a, Q, st)) return fail(c, "bowdb_query_stored_batch_dev: the query table does not fit the workgroup's LDS");
  LoopSelectArgs s;
  s.qframe = d_qframe; s.sharing = a.sharing; s.score = a.score; s.N = N; s.zero_tail = d_sharing ? 1 : 0; s.ratio = ratio; s.min_words = min_words;
  if (exclude_covisible) { s.row_ptr = db->cov_row; s.nbr = db->cov_nbr; s.rows = db->max_frames; }
  s.cand_frame = d_cand_frame; s.cand_sharing = d_cand_sharing; s.cand_score = d_cand_score; s.ccap = ccap; s.ncand = d_ncand; s.max_sharing = d_max_sharing;
  launch_loopdet_select(s, Q, st);
  note_launch(c, ST_BOW);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int airfe_bowdb_query_stored_batch_dev(airfe_bowdb* db, const int32_t* d_qframe, int Q, float ratio, int min_words, int exclude_covisible,
                                       int32_t* d_cand_frame, int32_t* d_cand_sharing, double* d_cand_score, int ccap, int* d_ncand, int* d_max_sharing,
                                       int32_t* d_sharing, void* stream) try {
  if (!db) return 1;
  airfe_ctx* c = db->c;
  AIRFE_ENTER(c);
  if (Q < 1 || ccap < 1 || !d_qframe || !d_cand_frame || !d_cand_sharing || !d_cand_score || !d_ncand || !d_max_sharing)
    return fail(c, "bowdb_query_stored_batch_dev: bad argument");
  if (Q > LD_MAX_QUERIES) return fail(c, "bowdb_query_stored_batch_dev: Q > 4096");
  if (exclude_covisible && !db->has_map) return fail(c, "bowdb_query_stored_batch_dev: exclude_covisible needs the map state (airfe_bowdb_attach_map)");
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  Carve k;
  const size_t qc = (size_t)Q * db->cap, o_vals = k.take(qc * 8), o_ids = k.take(qc * 4), o_nw = k.take((size_t)Q * 4);
  if (k.into(c, db->l_scratch, st)) return 1;
  return loopdet_query_queue(db, d_qframe, Q, ratio, min_words, exclude_covisible, k.at<uint32_t>(o_ids), k.d(o_vals), k.i(o_nw), d_cand_frame, d_cand_sharing,
                             d_cand_score, ccap, d_ncand, d_max_sharing, d_sharing, st);
} AIRFE_CATCH(db->c)

int airfe_loop_detect_batch_dev(airfe_ctx* c, airfe_bowdb* db, const airfe_loop_cfg* cfg, const int32_t* d_qframe, int Q, int* d_ok, int* d_stage,
                                int32_t* d_loop, double* d_Twq, double* d_Rlq, double* d_tlq, int* d_num, uint8_t* d_mask, int32_t* d_idx, float* d_score,
                                int mcap, int* d_nmatch, int* d_ncons, void* stream) try {
  AIRFE_ENTER(c);
  if (!db || db->c != c) return fail(c, "loop_detect_batch_dev: the database belongs to another context");
  if (!db->has_map) return fail(c, "loop_detect_batch_dev: no map state (airfe_bowdb_attach_map)");
  if (!db->has_pose) return fail(c, "loop_detect_batch_dev: the keyframe poses were never set (airfe_bowdb_set_poses)");
  if (!cfg || Q < 1 || mcap < 1 || !d_qframe || !d_ok || !d_stage || !d_loop || !d_Twq || !d_Rlq || !d_tlq || !d_num || !d_mask || !d_idx || !d_score ||
      !d_nmatch)
    return fail(c, "loop_detect_batch_dev: bad argument");
  if (cfg->K < 1 || cfg->K > 5) return fail(c, "loop_detect_batch_dev: cfg.K = 1..5");
  if (Q > LD_MAX_QUERIES) return fail(c, "loop_detect_batch_dev: Q > 4096");
  if (mcap > PO_MAX_POINTS) return fail(c, "loop_detect_batch_dev: mcap > 1024");
  if ((long long)Q * cfg->K > c->Pmax) return fail(c, "loop_detect_batch_dev: Q * K pairs exceed cfg.max_batch");
  const int N = db->size, ccap = std::max(N, 1), K = cfg->K, cap = db->cap;
  if (N > LD_MAX_FRAMES) return fail(c, "loop_detect_batch_dev: more than 4096 frames in the database");
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  // one block, every part 256-byte aligned
  Carve k;
  const size_t qc = (size_t)Q * cap, qm = (size_t)Q * mcap, qcc = (size_t)Q * ccap, qb = (size_t)Q * 4;
  const size_t o_ids = k.take(qc * 4), o_vals = k.take(qc * 8), o_nw = k.take(qb), o_cf = k.take(qcc * 4), o_cs = k.take(qcc * 4), o_sc = k.take(qcc * 8), o_nc = k.take(qb),
               o_ms = k.take(qb), o_odom = k.take((size_t)ccap * 8), o_feat = k.take(qc * AIRFE_FEAT_DIM * 4), o_qn = k.take(qb), o_qpos = k.take((size_t)Q * 24),
               o_md = k.take((size_t)Q * 8), o_T0 = k.take((size_t)Q * 128), o_gf = k.take((size_t)Q * K * 4), o_gs = k.take((size_t)Q * K * 8), o_ng = k.take(qb),
               o_gst = k.take(qb), o_map = k.take(qm * 4), o_X = k.take(qm * 24), o_obs = k.take(qm * 24), o_n = k.take(qb), o_nopt = k.take(qb), o_pre = k.take(qb);
  if (k.into(c, db->l_scratch, st)) return 1;
  // map_refiner.cc:97-130 on the database of :88-89: frame fq against its predecessors, the covisible frames dropped
  if (loopdet_query_queue(db, d_qframe, Q, cfg->ratio, cfg->min_words, 1, k.at<uint32_t>(o_ids), k.d(o_vals), k.i(o_nw), k.i(o_cf), k.i(o_cs),
                          k.d(o_sc), ccap, k.i(o_nc), k.i(o_ms), nullptr, st)) return 1;
  // :66-81: the odometry length, once per call; what the later steps read of frame fq
  launch_loopdet_odom(db->pos, N, k.d(o_odom), st);
  LoopStateArgs s;
  s.qframe = d_qframe; s.N = N; s.cap = cap; s.db_feat = db->feat; s.db_n = db->n; s.pos = db->pos; s.pose = db->pose; s.odom = k.d(o_odom);
  s.distance_rate = cfg->distance_rate; s.qfeat = k.at<float>(o_feat); s.qn = k.i(o_qn); s.qpos = k.d(o_qpos); s.max_dist = k.d(o_md);
  s.Twc0 = k.d(o_T0);
  launch_loopdet_state(s, Q, st);
  HIPCHK(c, hipGetLastError());
  // :132-214: the grouping in loop form; :213-230: the matcher over the K deputies
  if (bowdb_group_queue(db, BG_MODE_LOOP, k.i(o_cf), k.d(o_sc), k.i(o_nc), Q, ccap, K, nullptr, k.d(o_qpos), k.d(o_md), k.i(o_gf), k.d(o_gs), k.i(o_ng), k.i(o_gst), st)) return 1;
  if (bowdb_match_queue(c, db, s.qfeat, s.qn, Q, cap, k.i(o_gf), K, cfg->outlier_rejection, d_loop, d_idx, d_score, mcap, d_nmatch, nullptr, st)) return 1;
  // :232, :241-301: the gates and the constraints
  LoopGatherArgs g;
  g.qframe = d_qframe; g.xyz = db->xyz; g.u_right = db->u_right; g.feat = db->feat; g.N = N; g.cap = cap; g.best = d_loop; g.idx = d_idx; g.nmatch = d_nmatch;
  g.mcap = mcap; g.ncand = k.i(o_nc); g.gstatus = k.i(o_gst); g.ngroups = k.i(o_ng); g.min_matches = cfg->min_matches; g.min_points = cfg->min_points;
  g.X = k.d(o_X); g.obs = k.d(o_obs); g.map = k.i(o_map); g.n = k.i(o_n); g.n_opt = k.i(o_nopt); g.pre = k.i(o_pre);
  launch_loopdet_gather(g, Q, st);
  HIPCHK(c, hipGetLastError());
  // :262, :304: the frame optimisation from the stored pose, Tcb = identity; without constraints the kernel returns its start pose
  if (poseopt_queue(c, g.X, g.obs, g.n_opt, Q, mcap, k.d(o_T0), cfg->cam, nullptr, cfg->thr, d_Twq, nullptr, d_mask, mcap, g.map, d_num, -1, nullptr, st))
    return 1;
  // :308, :327-333
  LoopFinishArgs f;
  f.pre = g.pre; f.ncons = g.n; f.num = d_num; f.min_points = cfg->min_points; f.min_inliers = cfg->min_inliers; f.best = d_loop; f.N = N;
  f.pose = db->pose; f.Twq = d_Twq; f.stage = d_stage; f.ok = d_ok; f.ncons_out = d_ncons; f.Rlq = d_Rlq; f.tlq = d_tlq;
  launch_loopdet_finish(f, Q, st);
  HIPCHK(c, hipGetLastError());
  return 0;
} AIRFE_CATCH(c)

/* ---- map-point ids and the covisibility build (include/airfe.h "Map-point ids and the covisibility build"; kernels_covis.hip, covis_core.h) ------- */
// the build's work arrays inside c_scratch: sized by the database and max_points alone, so the block reserved at attach is never replaced by a build
struct CovisWork {
  Carve k;
  size_t o_count, o_start, o_tile, o_packed, o_seg, o_rowcnt, o_info, zero_bytes;
  CovisWork(const airfe_bowdb* db) {
    const size_t rows = (size_t)db->max_frames * db->cap, pts = (size_t)db->max_points + 1;
    zero_bytes = (pts + 4) * 4;                                                          // count [max_points + 1], then valid / ignored / status
    o_count = k.take(zero_bytes); o_start = k.take(pts * 4); o_tile = k.take(((pts + CV_SCAN_TILE - 1) / CV_SCAN_TILE) * 4);
    o_packed = k.take(rows * 4); o_seg = k.take(rows * 4); o_rowcnt = k.take((size_t)db->max_frames * 4); o_info = k.take(16);
  }
};

static int covis_build_queue(airfe_bowdb* db, int32_t* d_info, hipStream_t st, const char* who, int32_t** own_info) {
  airfe_ctx* c = db->c;
  if (!db->point_id) return fail(c, std::string(who) + ": no id table (airfe_bowdb_attach_point_ids)");
  if (db->size > CV_MAX_FRAMES) return fail(c, std::string(who) + ": more than 4096 frames in the database");
  CovisWork w(db);
  if (w.k.into(c, db->c_scratch, st)) return 1;
  if (own_info) *own_info = d_info = w.k.at<int32_t>(w.o_info);
  CovisArgs a;
  a.point_id = db->point_id; a.n = db->n; a.size = db->size; a.max_frames = db->max_frames; a.cap = db->cap; a.max_points = db->max_points;
  a.max_edges = db->max_edges;
  a.count = w.k.i(w.o_count); a.acc = a.count + (size_t)db->max_points + 1; a.start = w.k.i(w.o_start); a.tile = w.k.i(w.o_tile);
  a.packed = w.k.i(w.o_packed); a.seg = w.k.i(w.o_seg); a.rowcnt = w.k.i(w.o_rowcnt);
  a.row_ptr = db->cov_row; a.nbr = db->cov_nbr; a.weight = db->cov_weight; a.info = d_info;
  HIPCHK(c, hipMemsetAsync(a.count, 0, w.zero_bytes, st));
  launch_covis_build(a, st);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// rows first_frame .. first_frame + B - 1 of the id table
static int point_ids_copy(airfe_bowdb* db, int first_frame, int B, const int32_t* src, int32_t* dst, hipMemcpyKind kind, hipStream_t st, const char* who) {
  airfe_ctx* c = db->c;
  if (!db->point_id) return fail(c, std::string(who) + ": no id table (airfe_bowdb_attach_point_ids)");
  if (first_frame < 0 || B < 1 || B > db->max_frames - first_frame || (!src && !dst)) return fail(c, std::string(who) + ": bad argument (frames beyond max_frames)");
  const size_t n = (size_t)B * db->cap;
  if (src && kind == hipMemcpyHostToDevice)
    for (size_t i = 0; i < n; ++i)
      if (src[i] < -1 || src[i] >= db->max_points) return fail(c, std::string(who) + ": an id is < -1 or >= max_points (nothing was changed)");
  int32_t* at = db->point_id + (size_t)first_frame * db->cap;
  if (src) HIPCHK(c, hipMemcpyAsync(at, src, n * 4, kind, st));
  else HIPCHK(c, hipMemcpyAsync(dst, at, n * 4, kind, st));
  if (kind != hipMemcpyDeviceToDevice) HIPCHK(c, hipStreamSynchronize(st));
  return 0;
}
int airfe_bowdb_attach_point_ids(airfe_bowdb* db, int max_points) try {
  if (!db) return 1;
  airfe_ctx* c = db->c;
  AIRFE_ENTER(c);
  if (!db->has_map) return fail(c, "bowdb_attach_point_ids: no map state (airfe_bowdb_attach_map)");
  if (db->point_id) return fail(c, "bowdb_attach_point_ids: the id table is attached already");
  if (max_points < 1 || max_points > CV_MAX_POINTS) return fail(c, "bowdb_attach_point_ids: max_points must be 1 .. 16777216");
  const size_t rows = (size_t)db->max_frames * db->cap;
  int32_t* ids = nullptr;
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&ids), rows * 4));
  db->max_points = max_points;
  CovisWork w(db);
  if (w.k.into(c, db->c_scratch, c->stream) || hipMemsetAsync(ids, 0xFF, rows * 4, c->stream) != hipSuccess ||      // every byte 0xFF: -1 in every slot
      hipStreamSynchronize(c->stream) != hipSuccess) {
    (void)hipFree(ids);
    db->max_points = 0;
    return fail(c, "bowdb_attach_point_ids: out of device memory");
  }
  db->point_id = ids;
  return 0;
} AIRFE_CATCH(db->c)

int airfe_bowdb_set_point_ids_dev(airfe_bowdb* db, int first_frame, int B, const int32_t* d_ids, void* stream) try {
  if (!db) return 1;
  AIRFE_ENTER(db->c);
  return point_ids_copy(db, first_frame, B, d_ids, nullptr, hipMemcpyDeviceToDevice, stream ? (hipStream_t)stream : db->c->stream, "bowdb_set_point_ids_dev");
} AIRFE_CATCH(db->c)

int airfe_bowdb_set_point_ids(airfe_bowdb* db, int first_frame, int B, const int32_t* ids) try {
  if (!db) return 1;
  AIRFE_ENTER(db->c);
  return point_ids_copy(db, first_frame, B, ids, nullptr, hipMemcpyHostToDevice, db->c->stream, "bowdb_set_point_ids");
} AIRFE_CATCH(db->c)

int airfe_bowdb_get_point_ids(airfe_bowdb* db, int first_frame, int B, int32_t* ids) try {
  if (!db) return 1;
  AIRFE_ENTER(db->c);
  return point_ids_copy(db, first_frame, B, nullptr, ids, hipMemcpyDeviceToHost, db->c->stream, "bowdb_get_point_ids");
} AIRFE_CATCH(db->c)

int airfe_bowdb_build_covisibility_dev(airfe_bowdb* db, int32_t* d_info, void* stream) try {
  if (!db) return 1;
  AIRFE_ENTER(db->c);
  if (!d_info) return fail(db->c, "bowdb_build_covisibility_dev: bad argument");
  return covis_build_queue(db, d_info, stream ? (hipStream_t)stream : db->c->stream, "bowdb_build_covisibility_dev", nullptr);
} AIRFE_CATCH(db->c)

int airfe_bowdb_build_covisibility(airfe_bowdb* db, int* n_edges) try {
  if (!db) return 1;
  airfe_ctx* c = db->c;
  AIRFE_ENTER(c);
  if (!n_edges) return fail(c, "bowdb_build_covisibility: bad argument");
  int32_t* d_info = nullptr;
  int32_t info[4] = {0, 0, 0, 0};
  if (covis_build_queue(db, nullptr, c->stream, "bowdb_build_covisibility", &d_info)) return 1;
  HIPCHK(c, hipMemcpyAsync(info, d_info, 16, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *n_edges = info[1];
  if (info[0]) return fail(c, "bowdb_build_covisibility: more entries than max_edges (the graph is empty now)");
  return 0;
} AIRFE_CATCH(db->c)

/* ---- map-point triangulation (include/airfe.h "Map-point triangulation"; kernels_triangulate.hip, triangulate_core.h) ------------------------------ */
// the triangulation's own arrays inside t_scratch, sized by the database and max_points alone: the segments as filled and sorted, and the host form's
// device outputs.  The marks and the segment starts are the covisibility build's work arrays (c_scratch), rewritten by either build.
struct TriWork {
  Carve k;
  size_t o_seg, o_sorted, o_xyz, o_status, o_nobs, o_info;
  TriWork(const airfe_bowdb* db) {
    const size_t rows = (size_t)db->max_frames * db->cap, pts = (size_t)db->max_points;
    o_seg = k.take(rows * 4); o_sorted = k.take(rows * 4); o_xyz = k.take(pts * 24); o_status = k.take(pts * 4); o_nobs = k.take(pts * 4); o_info = k.take(16);
  }
};

static int triangulate_queue(airfe_bowdb* db, const double* cam, int min_observers, double* d_xyz, int32_t* d_status, int32_t* d_nobs, int32_t* d_info,
                             hipStream_t st, const char* who) {
  airfe_ctx* c = db->c;
  if (!db->has_tri) return fail(c, std::string(who) + ": no triangulation attached (airfe_bowdb_attach_triangulation)");
  if (db->size > TR_MAX_FRAMES) return fail(c, std::string(who) + ": more than 4096 frames in the database");
  if (!cam || !d_xyz || !d_status || !d_nobs || !d_info) return fail(c, std::string(who) + ": bad argument");
  TriangulateArgs t;
  if (!tr_cam(cam, t.cami)) return fail(c, std::string(who) + ": fx and fy must be finite and not zero");
  CovisWork w(db);
  TriWork tw(db);
  if (w.k.into(c, db->c_scratch, st) || tw.k.into(c, db->t_scratch, st)) return 1;      // (reserved at attach: neither block is replaced here)
  CovisArgs a;
  a.point_id = db->point_id; a.n = db->n; a.size = db->size; a.max_frames = db->max_frames; a.cap = db->cap; a.max_points = db->max_points;
  a.count = w.k.i(w.o_count); a.acc = a.count + (size_t)db->max_points + 1; a.start = w.k.i(w.o_start); a.tile = w.k.i(w.o_tile);
  a.packed = w.k.i(w.o_packed);
  t.feat = db->feat; t.n = db->n; t.pose = db->pose; t.size = db->size; t.cap = db->cap; t.feat_dim = AIRFE_FEAT_DIM; t.max_points = db->max_points;
  t.min_observers = min_observers;
  t.packed = a.packed; t.start = a.start; t.count = a.count; t.seg = tw.k.i(tw.o_seg); t.sorted = tw.k.i(tw.o_sorted);
  t.xyz = d_xyz; t.status = d_status; t.nobs = d_nobs; t.info = d_info;
  HIPCHK(c, hipMemsetAsync(a.count, 0, w.zero_bytes, st));
  HIPCHK(c, hipMemsetAsync(d_info, 0, 16, st));
  if (db->size > 0) launch_covis_segments(a, st);
  launch_triangulate(t, st);
  HIPCHK(c, hipGetLastError());
  return 0;
}

static int fill_points_queue(airfe_bowdb* db, const double* d_xyz, const int32_t* d_status, int only_missing, int32_t* d_written, hipStream_t st,
                             const char* who) {
  airfe_ctx* c = db->c;
  if (!db->has_tri) return fail(c, std::string(who) + ": no triangulation attached (airfe_bowdb_attach_triangulation)");
  if (db->size > TR_MAX_FRAMES) return fail(c, std::string(who) + ": more than 4096 frames in the database");
  if (!d_xyz || !d_status || !d_written) return fail(c, std::string(who) + ": bad argument");
  FillPointsArgs f;
  f.point_id = db->point_id; f.n = db->n; f.size = db->size; f.cap = db->cap; f.max_points = db->max_points; f.only_missing = only_missing != 0;
  f.xyz = d_xyz; f.status = d_status; f.points = db->xyz; f.written = d_written;
  HIPCHK(c, hipMemsetAsync(d_written, 0, 4, st));
  launch_fill_points(f, st);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int airfe_bowdb_attach_triangulation(airfe_bowdb* db) try {
  if (!db) return 1;
  airfe_ctx* c = db->c;
  AIRFE_ENTER(c);
  if (!db->point_id) return fail(c, "bowdb_attach_triangulation: no id table (airfe_bowdb_attach_point_ids)");
  if (db->has_tri) return fail(c, "bowdb_attach_triangulation: the triangulation is attached already");
  TriWork tw(db);
  if (tw.k.into(c, db->t_scratch, c->stream)) return 1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  db->has_tri = 1;
  return 0;
} AIRFE_CATCH(db->c)

int airfe_bowdb_triangulate_points_dev(airfe_bowdb* db, const double* cam, int min_observers, double* d_xyz, int32_t* d_status, int32_t* d_nobs,
                                       int32_t* d_info, void* stream) try {
  if (!db) return 1;
  AIRFE_ENTER(db->c);
  return triangulate_queue(db, cam, min_observers, d_xyz, d_status, d_nobs, d_info, stream ? (hipStream_t)stream : db->c->stream,
                           "bowdb_triangulate_points_dev");
} AIRFE_CATCH(db->c)

int airfe_bowdb_triangulate_points(airfe_bowdb* db, const double* cam, int min_observers, double* xyz, int32_t* status, int32_t* nobs, int* n_ok) try {
  if (!db) return 1;
  airfe_ctx* c = db->c;
  AIRFE_ENTER(c);
  if (!db->has_tri) return fail(c, "bowdb_triangulate_points: no triangulation attached (airfe_bowdb_attach_triangulation)");
  if (!xyz || !status || !nobs || !n_ok) return fail(c, "bowdb_triangulate_points: bad argument");
  TriWork tw(db);
  if (tw.k.into(c, db->t_scratch, c->stream)) return 1;
  int32_t info[4] = {0, 0, 0, 0};
  if (triangulate_queue(db, cam, min_observers, tw.k.d(tw.o_xyz), tw.k.at<int32_t>(tw.o_status), tw.k.at<int32_t>(tw.o_nobs), tw.k.at<int32_t>(tw.o_info),
                        c->stream, "bowdb_triangulate_points"))
    return 1;
  const size_t P = (size_t)db->max_points;
  HIPCHK(c, hipMemcpyAsync(xyz, tw.k.d(tw.o_xyz), P * 24, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(status, tw.k.at<int32_t>(tw.o_status), P * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(nobs, tw.k.at<int32_t>(tw.o_nobs), P * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(info, tw.k.at<int32_t>(tw.o_info), 16, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *n_ok = info[0];
  return 0;
} AIRFE_CATCH(db->c)

int airfe_bowdb_fill_points_dev(airfe_bowdb* db, const double* d_xyz, const int32_t* d_status, int only_missing, int32_t* d_written, void* stream) try {
  if (!db) return 1;
  AIRFE_ENTER(db->c);
  return fill_points_queue(db, d_xyz, d_status, only_missing, d_written, stream ? (hipStream_t)stream : db->c->stream, "bowdb_fill_points_dev");
} AIRFE_CATCH(db->c)

int airfe_triangulate_point(const double* cam, const double* Twc, const float* xy, int n, double* xyz, int* status) try {
  double cami[4];
  if (!cam || !xyz || !status || n < 0 || (n > 0 && (!Twc || !xy))) return fail(nullptr, "triangulate_point: bad argument");
  if (!tr_cam(cam, cami)) return fail(nullptr, "triangulate_point: fx and fy must be finite and not zero");
  *status = triangulate_point_core(cami, Twc, xy, n, 2, xyz);      // (compiled beside the kernels, without contraction)
  return 0;
} AIRFE_CATCH(nullptr)

/* ---- relocalisation's junction term (include/airfe.h "Junction term"; kernels_junction.hip, junction_core.h) --------------------------------------- */
static int junction_connect_queue(airfe_ctx* c, const double* d_lines, const int* d_nlines, int capL, const float* d_junc, const int* d_njunc, int capJ, int B,
                                  int W, int H, int32_t* d_edge, int ecap, int* d_nedge, int* d_status, int32_t* d_line_pair, hipStream_t st) {
  JunctionConnectArgs a;
  a.lines = d_lines; a.nlines = d_nlines; a.capL = capL; a.junc = d_junc; a.njunc = d_njunc; a.capJ = capJ; a.W = W; a.H = H; a.ecap = ecap;
  a.edge = d_edge; a.nedge = d_nedge; a.status = d_status; a.line_pair = d_line_pair;
  launch_junction_connect(a, B, st);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// the tables of B frames into rows first .. of `tab` (the stored frames' or the queries'); out_word / out_nj: the stored copy of the words or nullptr
static int junction_keys_queue(airfe_bowdb* db, const airfe_bowdb::JunctionTables& tab, int first, int B, const uint32_t* d_word, const int* d_nj,
                               const int32_t* d_edge, const int* d_nedge, const int* d_status, unsigned* out_word, int* out_nj, hipStream_t st) {
  JunctionKeysArgs a;
  a.word = d_word; a.nj = d_nj; a.cap = db->cap; a.edge = d_edge; a.nedge = d_nedge; a.ecap = db->j_ecap; a.status_in = d_status; a.first = first;
  a.out_word = out_word; a.out_nj = out_nj; a.uword = tab.uword; a.wcnt = tab.wcnt; a.wconn = tab.wconn; a.nuw = tab.nuw; a.ukey = tab.ukey; a.kcnt = tab.kcnt;
  a.nuk = tab.nuk; a.status = tab.status;
  launch_junction_keys(a, B, st);
  HIPCHK(db->c, hipGetLastError());
  return 0;
}

// the queries' tables, the unchanged bowdb_query_kernel for the dense score, the term
static int junction_term_queue(airfe_bowdb* db, const uint32_t* d_ids, const double* d_vals, const int* d_nw, const uint32_t* d_word, const int* d_nj,
                               const int32_t* d_edge, const int* d_nedge, const int* d_qstatus, int Q, double* d_extra, int32_t* d_match_num,
                               int32_t* d_line_match_num, hipStream_t st) {
  airfe_ctx* c = db->c;
  const int N = db->size;
  if (junction_keys_queue(db, db->j_queries, 0, Q, d_word, d_nj, d_edge, d_nedge, d_qstatus, nullptr, nullptr, st)) return 1;
  BowQueryArgs q;
  q.db_ids = db->ids; q.db_vals = db->vals; q.db_nw = db->nw; q.N = N; q.cap = db->cap;
  q.q_ids = d_ids; q.q_vals = d_vals; q.q_nw = d_nw; q.qcap = db->cap; q.n_words = c->bow_nwords;
  q.frames_per_wg = (size_t)Q * N >= (size_t)64 * 1024 ? 64 : 16;
  q.score = db->j_score; q.sharing = db->j_sharing;
  if (launch_bowdb_query(q, Q, st)) return fail(c, "bowdb_junction_term_batch_dev: the query table does not fit the workgroup's LDS");
  JunctionTermArgs a;
  const airfe_bowdb::JunctionTables &tq = db->j_queries, &tf = db->j_frames;
  a.q_uword = tq.uword; a.q_wconn = tq.wconn; a.q_nuw = tq.nuw; a.q_ukey = tq.ukey; a.q_kcnt = tq.kcnt; a.q_nuk = tq.nuk; a.q_status = tq.status;
  a.f_uword = tf.uword; a.f_wcnt = tf.wcnt; a.f_nuw = tf.nuw; a.f_ukey = tf.ukey; a.f_kcnt = tf.kcnt; a.f_nuk = tf.nuk; a.f_status = tf.status;
  a.N = N; a.cap = db->cap; a.ecap = db->j_ecap; a.frames_per_wg = q.frames_per_wg; a.score = db->j_score;
  a.extra = d_extra; a.match_num = d_match_num; a.line_match_num = d_line_match_num;
  launch_junction_term(a, Q, st);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int airfe_junction_connections_batch_dev(airfe_ctx* c, const double* d_lines, const int* d_nlines, int capL, const float* d_junc, const int* d_njunc, int capJ,
                                         int B, int W, int H, int32_t* d_edge, int ecap, int* d_nedge, int* d_status, int32_t* d_line_pair,
                                         void* stream) try {
  AIRFE_ENTER(c);
  if (B < 1 || capL < 1 || capJ < 1 || W < 1 || H < 1 || ecap < 1 || !d_lines || !d_nlines || !d_junc || !d_njunc || !d_edge || !d_nedge || !d_status)
    return fail(c, "junction_connections_batch_dev: bad argument");
  if (capJ > JN_MAX_JUNCTIONS) return fail(c, "junction_connections_batch_dev: capJ > 1024");
  if (ecap > JN_MAX_EDGES) return fail(c, "junction_connections_batch_dev: ecap > 4096");
  return junction_connect_queue(c, d_lines, d_nlines, capL, d_junc, d_njunc, capJ, B, W, H, d_edge, ecap, d_nedge, d_status, d_line_pair,
                                stream ? (hipStream_t)stream : c->stream);
} AIRFE_CATCH(c)

int airfe_junction_connections(airfe_ctx* c, const double* lines, int nl, const float* junc, int nj, int W, int H, int32_t* edge, int ecap, int* nedge,
                               int32_t* line_pair) try {
  if (!c) return 1;
  if (nl < 0 || nj < 0 || W < 1 || H < 1 || ecap < 1 || !nedge || !edge || (nl > 0 && !lines) || (nj > 0 && !junc))
    return fail(c, "junction_connections: bad argument");
  if (ecap > JN_MAX_EDGES) return fail(c, "junction_connections: ecap > 4096");
  if (jn_connections_host(lines, nl, junc, nj, W, H, edge, ecap, nedge, line_pair) != JN_OK) {
    (void)fail(c, "junction_connections: more than ecap distinct edges or more than 1024 junctions (status 2: the frame has no edges)");
    return JN_OVERFLOW;
  }
  return 0;
} AIRFE_CATCH(c)

int airfe_bowdb_attach_junctions(airfe_bowdb* db, int ecap, int max_queries) try {
  if (!db) return 1;
  airfe_ctx* c = db->c;
  AIRFE_ENTER(c);
  if (db->j_ecap) return fail(c, "bowdb_attach_junctions: the junction state is attached already");
  if (ecap < 1 || max_queries < 1) return fail(c, "bowdb_attach_junctions: bad argument");
  if (ecap > JN_MAX_EDGES) return fail(c, "bowdb_attach_junctions: ecap > 4096");
  const size_t F = (size_t)db->max_frames, Qm = (size_t)max_queries, cap = (size_t)db->cap, E = (size_t)ecap;
  Carve k;
  struct Off { size_t uword, wcnt, wconn, nuw, ukey, kcnt, nuk, status; } o[2];
  for (int s = 0; s < 2; ++s) {
    const size_t R = s == 0 ? F : Qm;
    o[s].ukey = k.take(R * E * 8); o[s].kcnt = k.take(R * E * 4); o[s].uword = k.take(R * cap * 4); o[s].wcnt = k.take(R * cap * 4);
    o[s].wconn = k.take(R * cap * 4); o[s].nuw = k.take(R * 4); o[s].nuk = k.take(R * 4); o[s].status = k.take(R * 4);
  }
  const size_t o_word = k.take(F * cap * 4), o_nj = k.take(F * 4), o_score = k.take(Qm * F * 8), o_sharing = k.take(Qm * F * 4), o_vals = k.take(Qm * cap * 8),
               o_ids = k.take(Qm * cap * 4), o_qword = k.take(Qm * cap * 4), o_edge = k.take(Qm * E * 8), o_nw = k.take(Qm * 4), o_qnj = k.take(Qm * 4),
               o_nedge = k.take(Qm * 4), o_qst = k.take(Qm * 4);
  if (k.into(c, db->j_block, c->stream)) return 1;
  HIPCHK(c, hipMemsetAsync(db->j_block.p, 0, k.size(), c->stream));
  airfe_bowdb::JunctionTables* t[2] = {&db->j_frames, &db->j_queries};
  for (int s = 0; s < 2; ++s) {
    t[s]->ukey = k.at<unsigned long long>(o[s].ukey); t[s]->kcnt = k.i(o[s].kcnt); t[s]->uword = k.at<unsigned>(o[s].uword); t[s]->wcnt = k.i(o[s].wcnt);
    t[s]->wconn = k.i(o[s].wconn); t[s]->nuw = k.i(o[s].nuw); t[s]->nuk = k.i(o[s].nuk); t[s]->status = k.i(o[s].status);
  }
  db->j_word = k.at<unsigned>(o_word); db->j_nj = k.i(o_nj); db->j_score = k.d(o_score); db->j_sharing = k.i(o_sharing); db->j_vals = k.d(o_vals);
  db->j_ids = k.at<unsigned>(o_ids); db->j_qword = k.at<unsigned>(o_qword); db->j_edge = k.at<int32_t>(o_edge); db->j_nw = k.i(o_nw); db->j_qnj = k.i(o_qnj);
  db->j_nedge = k.i(o_nedge); db->j_qstatus = k.i(o_qst);
  HIPCHK(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(db->j_frames.status), JN_UNSET, F, c->stream));      // no frame has junction state yet
  HIPCHK(c, hipStreamSynchronize(c->stream));
  db->j_maxq = max_queries;
  db->j_ecap = ecap;
  return 0;
} AIRFE_CATCH(db->c)

int airfe_bowdb_set_junctions_dev(airfe_bowdb* db, int first_frame, int B, const uint32_t* d_word, const int* d_nj, const int32_t* d_edge, const int* d_nedge,
                                  const int* d_status, void* stream) try {
  if (!db) return 1;
  airfe_ctx* c = db->c;
  AIRFE_ENTER(c);
  if (!db->j_ecap) return fail(c, "bowdb_set_junctions_dev: no junction state (airfe_bowdb_attach_junctions)");
  if (first_frame < 0 || B < 1 || B > db->max_frames - first_frame || !d_word || !d_nj || !d_edge || !d_nedge)
    return fail(c, "bowdb_set_junctions_dev: bad argument (frames beyond max_frames)");
  return junction_keys_queue(db, db->j_frames, first_frame, B, d_word, d_nj, d_edge, d_nedge, d_status, db->j_word, db->j_nj,
                             stream ? (hipStream_t)stream : c->stream);
} AIRFE_CATCH(db->c)

int airfe_bowdb_set_junctions(airfe_bowdb* db, int first_frame, int B, const uint32_t* word, const int* nj, const int32_t* edge, const int* nedge,
                              const int* status) try {
  if (!db) return 1;
  airfe_ctx* c = db->c;
  AIRFE_ENTER(c);
  if (!db->j_ecap) return fail(c, "bowdb_set_junctions: no junction state (airfe_bowdb_attach_junctions)");
  if (first_frame < 0 || B < 1 || B > db->max_frames - first_frame || !word || !nj || !edge || !nedge)
    return fail(c, "bowdb_set_junctions: bad argument (frames beyond max_frames)");
  if (B > db->j_maxq) return fail(c, "bowdb_set_junctions: more than max_queries frames in one call (the staging is sized by it)");
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemcpyAsync(db->j_qword, word, (size_t)B * db->cap * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(db->j_qnj, nj, (size_t)B * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(db->j_edge, edge, (size_t)B * db->j_ecap * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(db->j_nedge, nedge, (size_t)B * 4, hipMemcpyHostToDevice, st));
  if (status) HIPCHK(c, hipMemcpyAsync(db->j_qstatus, status, (size_t)B * 4, hipMemcpyHostToDevice, st));
  if (junction_keys_queue(db, db->j_frames, first_frame, B, db->j_qword, db->j_qnj, db->j_edge, db->j_nedge, status ? db->j_qstatus : nullptr, db->j_word,
                          db->j_nj, st)) return 1;
  HIPCHK(c, hipStreamSynchronize(st));
  return 0;
} AIRFE_CATCH(db->c)

int airfe_bowdb_get_junctions(airfe_bowdb* db, int first_frame, int B, uint32_t* word, int* nj, uint32_t* uword, int32_t* wcnt, int32_t* wconn, int* nuw,
                              uint64_t* ukey, int32_t* kcnt, int* nuk, int* status) try {
  if (!db) return 1;
  airfe_ctx* c = db->c;
  AIRFE_ENTER(c);
  if (!db->j_ecap) return fail(c, "bowdb_get_junctions: no junction state (airfe_bowdb_attach_junctions)");
  if (first_frame < 0 || B < 1 || B > db->max_frames - first_frame) return fail(c, "bowdb_get_junctions: bad argument (frames beyond max_frames)");
  hipStream_t st = c->stream;
  const size_t f = (size_t)first_frame, cap = (size_t)db->cap, E = (size_t)db->j_ecap, n = (size_t)B;
  const airfe_bowdb::JunctionTables& t = db->j_frames;
  if (word) HIPCHK(c, hipMemcpyAsync(word, db->j_word + f * cap, n * cap * 4, hipMemcpyDeviceToHost, st));
  if (nj) HIPCHK(c, hipMemcpyAsync(nj, db->j_nj + f, n * 4, hipMemcpyDeviceToHost, st));
  if (uword) HIPCHK(c, hipMemcpyAsync(uword, t.uword + f * cap, n * cap * 4, hipMemcpyDeviceToHost, st));
  if (wcnt) HIPCHK(c, hipMemcpyAsync(wcnt, t.wcnt + f * cap, n * cap * 4, hipMemcpyDeviceToHost, st));
  if (wconn) HIPCHK(c, hipMemcpyAsync(wconn, t.wconn + f * cap, n * cap * 4, hipMemcpyDeviceToHost, st));
  if (nuw) HIPCHK(c, hipMemcpyAsync(nuw, t.nuw + f, n * 4, hipMemcpyDeviceToHost, st));
  if (ukey) HIPCHK(c, hipMemcpyAsync(ukey, t.ukey + f * E, n * E * 8, hipMemcpyDeviceToHost, st));
  if (kcnt) HIPCHK(c, hipMemcpyAsync(kcnt, t.kcnt + f * E, n * E * 4, hipMemcpyDeviceToHost, st));
  if (nuk) HIPCHK(c, hipMemcpyAsync(nuk, t.nuk + f, n * 4, hipMemcpyDeviceToHost, st));
  if (status) HIPCHK(c, hipMemcpyAsync(status, t.status + f, n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return 0;
} AIRFE_CATCH(db->c)

int airfe_bowdb_junction_term_batch_dev(airfe_bowdb* db, const uint32_t* d_ids, const double* d_vals, const int* d_nw, const uint32_t* d_word, const int* d_nj,
                                        const int32_t* d_edge, const int* d_nedge, const int* d_qstatus, int Q, double* d_extra, int32_t* d_match_num,
                                        int32_t* d_line_match_num, void* stream) try {
  if (!db) return 1;
  airfe_ctx* c = db->c;
  AIRFE_ENTER(c);
  if (!db->j_ecap) return fail(c, "bowdb_junction_term_batch_dev: no junction state (airfe_bowdb_attach_junctions)");
  if (Q < 1 || !d_ids || !d_vals || !d_nw || !d_word || !d_nj || !d_edge || !d_nedge || !d_extra) return fail(c, "bowdb_junction_term_batch_dev: bad argument");
  if (Q > db->j_maxq) return fail(c, "bowdb_junction_term_batch_dev: Q > max_queries");
  return junction_term_queue(db, d_ids, d_vals, d_nw, d_word, d_nj, d_edge, d_nedge, d_qstatus, Q, d_extra, d_match_num, d_line_match_num,
                             stream ? (hipStream_t)stream : c->stream);
} AIRFE_CATCH(db->c)

// the checks the two composites share
static int junction_chain_check(airfe_bowdb* db, const float* d_junc, const int* d_njunc, int capJ, const double* d_lines, const int* d_nlines, int capL, int B,
                                int W, int H, const char* who) {
  airfe_ctx* c = db->c;
  if (!db->j_ecap) return fail(c, std::string(who) + ": no junction state (airfe_bowdb_attach_junctions)");
  if (B < 1 || capL < 1 || W < 1 || H < 1 || !d_junc || !d_njunc || !d_lines || !d_nlines) return fail(c, std::string(who) + ": bad argument");
  if (capJ > JN_MAX_JUNCTIONS) return fail(c, std::string(who) + ": capJ > 1024");
  if (capJ != db->cap) return fail(c, std::string(who) + ": capJ must be the database's cap");
  if (B > db->j_maxq) return fail(c, std::string(who) + ": more than max_queries frames in one call");
  if (!c->bow_nodes) return fail(c, std::string(who) + ": no vocabulary loaded (airfe_bow_load)");
  return 0;
}

int airfe_bowdb_junction_extra_batch_dev(airfe_bowdb* db, const float* d_junc, const int* d_njunc, int capJ, const double* d_lines, const int* d_nlines,
                                         int capL, int Q, int W, int H, double* d_extra, int32_t* d_match_num, int32_t* d_line_match_num, void* stream) try {
  if (!db) return 1;
  airfe_ctx* c = db->c;
  AIRFE_ENTER(c);
  if (junction_chain_check(db, d_junc, d_njunc, capJ, d_lines, d_nlines, capL, Q, W, H, "bowdb_junction_extra_batch_dev")) return 1;
  if (!d_extra) return fail(c, "bowdb_junction_extra_batch_dev: bad argument");
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  // map_user.cc:133: the junction vector and the words; :287: the connections; :290-331: the term
  if (bow_vector_queue(c, d_junc, d_njunc, Q, capJ, db->j_ids, db->j_vals, db->j_nw, db->j_qword, st)) return 1;
  if (junction_connect_queue(c, d_lines, d_nlines, capL, d_junc, d_njunc, capJ, Q, W, H, db->j_edge, db->j_ecap, db->j_nedge, db->j_qstatus, nullptr, st))
    return 1;
  return junction_term_queue(db, db->j_ids, db->j_vals, db->j_nw, db->j_qword, d_njunc, db->j_edge, db->j_nedge, db->j_qstatus, Q, d_extra, d_match_num,
                             d_line_match_num, st);
} AIRFE_CATCH(db->c)

int airfe_bowdb_add_junction_frames_batch_dev(airfe_bowdb* db, const float* d_junc, const int* d_njunc, int capJ, const double* d_lines, const int* d_nlines,
                                              int capL, int B, int W, int H, void* stream) try {
  if (!db) return 1;
  airfe_ctx* c = db->c;
  AIRFE_ENTER(c);
  if (junction_chain_check(db, d_junc, d_njunc, capJ, d_lines, d_nlines, capL, B, W, H, "bowdb_add_junction_frames_batch_dev")) return 1;
  if (B > db->max_frames - db->size) return fail(c, "bowdb_add_junction_frames_batch_dev: the database is full (max_frames)");
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  const int first = db->size;
  // map_refiner.cc:986-994: FrameToBow + AddFrame per keyframe; frame.cc:581-629 for the same frames
  if (bow_vector_queue(c, d_junc, d_njunc, B, capJ, db->j_ids, db->j_vals, db->j_nw, db->j_qword, st)) return 1;
  if (bowdb_add_impl(db, db->j_ids, db->j_vals, db->j_nw, d_junc, d_njunc, B, capJ, hipMemcpyDeviceToDevice, st, "bowdb_add_junction_frames_batch_dev")) return 1;
  if (junction_connect_queue(c, d_lines, d_nlines, capL, d_junc, d_njunc, capJ, B, W, H, db->j_edge, db->j_ecap, db->j_nedge, db->j_qstatus, nullptr, st))
    return 1;
  return junction_keys_queue(db, db->j_frames, first, B, db->j_qword, d_njunc, db->j_edge, db->j_nedge, db->j_qstatus, db->j_word, db->j_nj, st);
} AIRFE_CATCH(db->c)

}  // extern "C"
