// airfe — relocalisation's junction term (include/airfe.h "Junction term"): the junction connections, the database's junction tables, the term and its two
// composites (kernels_junction.hip, junction_core.h).
#include "airfe_bowdb.h"
#include "junction_core.h"

extern "C" {

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
  JunctionTermArgs a;
  if (bowdb_dense_query_queue(db, d_ids, d_vals, d_nw, Q, db->cap, db->j_score, db->j_sharing, &a.frames_per_wg, st, "bowdb_junction_term_batch_dev")) return 1;
  const airfe_bowdb::JunctionTables &tq = db->j_queries, &tf = db->j_frames;
  a.q_uword = tq.uword; a.q_wconn = tq.wconn; a.q_nuw = tq.nuw; a.q_ukey = tq.ukey; a.q_kcnt = tq.kcnt; a.q_nuk = tq.nuk; a.q_status = tq.status;
  a.f_uword = tf.uword; a.f_wcnt = tf.wcnt; a.f_nuw = tf.nuw; a.f_ukey = tf.ukey; a.f_kcnt = tf.kcnt; a.f_nuk = tf.nuk; a.f_status = tf.status;
  a.N = N; a.cap = db->cap; a.ecap = db->j_ecap; a.score = db->j_score;      // (frames_per_wg: the dense query's, set above)
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
  return junction_connect_queue(c, d_lines, d_nlines, capL, d_junc, d_njunc, capJ, B, W, H, d_edge, ecap, d_nedge, d_status, d_line_pair, stream_of(c, stream));
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
  BOWDB_ENTER(db);
  airfe_ctx* c = db->c;
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
  BOWDB_ENTER(db);
  airfe_ctx* c = db->c;
  if (!db->j_ecap) return fail(c, "bowdb_set_junctions_dev: no junction state (airfe_bowdb_attach_junctions)");
  if (first_frame < 0 || B < 1 || B > db->max_frames - first_frame || !d_word || !d_nj || !d_edge || !d_nedge)
    return fail(c, "bowdb_set_junctions_dev: bad argument (frames beyond max_frames)");
  return junction_keys_queue(db, db->j_frames, first_frame, B, d_word, d_nj, d_edge, d_nedge, d_status, db->j_word, db->j_nj, stream_of(c, stream));
} AIRFE_CATCH(db->c)

int airfe_bowdb_set_junctions(airfe_bowdb* db, int first_frame, int B, const uint32_t* word, const int* nj, const int32_t* edge, const int* nedge,
                              const int* status) try {
  BOWDB_ENTER(db);
  airfe_ctx* c = db->c;
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
  BOWDB_ENTER(db);
  airfe_ctx* c = db->c;
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
  BOWDB_ENTER(db);
  airfe_ctx* c = db->c;
  if (!db->j_ecap) return fail(c, "bowdb_junction_term_batch_dev: no junction state (airfe_bowdb_attach_junctions)");
  if (Q < 1 || !d_ids || !d_vals || !d_nw || !d_word || !d_nj || !d_edge || !d_nedge || !d_extra) return fail(c, "bowdb_junction_term_batch_dev: bad argument");
  if (Q > db->j_maxq) return fail(c, "bowdb_junction_term_batch_dev: Q > max_queries");
  return junction_term_queue(db, d_ids, d_vals, d_nw, d_word, d_nj, d_edge, d_nedge, d_qstatus, Q, d_extra, d_match_num, d_line_match_num, stream_of(c, stream));
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
  BOWDB_ENTER(db);
  airfe_ctx* c = db->c;
  if (junction_chain_check(db, d_junc, d_njunc, capJ, d_lines, d_nlines, capL, Q, W, H, "bowdb_junction_extra_batch_dev")) return 1;
  if (!d_extra) return fail(c, "bowdb_junction_extra_batch_dev: bad argument");
  hipStream_t st = stream_of(c, stream);
  // map_user.cc:133: the junction vector and the words; :287: the connections; :290-331: the term
  if (bow_vector_queue(c, d_junc, d_njunc, Q, capJ, db->j_ids, db->j_vals, db->j_nw, db->j_qword, st)) return 1;
  if (junction_connect_queue(c, d_lines, d_nlines, capL, d_junc, d_njunc, capJ, Q, W, H, db->j_edge, db->j_ecap, db->j_nedge, db->j_qstatus, nullptr, st))
    return 1;
  return junction_term_queue(db, db->j_ids, db->j_vals, db->j_nw, db->j_qword, d_njunc, db->j_edge, db->j_nedge, db->j_qstatus, Q, d_extra, d_match_num,
                             d_line_match_num, st);
} AIRFE_CATCH(db->c)

int airfe_bowdb_add_junction_frames_batch_dev(airfe_bowdb* db, const float* d_junc, const int* d_njunc, int capJ, const double* d_lines, const int* d_nlines,
                                              int capL, int B, int W, int H, void* stream) try {
  BOWDB_ENTER(db);
  airfe_ctx* c = db->c;
  if (junction_chain_check(db, d_junc, d_njunc, capJ, d_lines, d_nlines, capL, B, W, H, "bowdb_add_junction_frames_batch_dev")) return 1;
  if (B > db->max_frames - db->size) return fail(c, "bowdb_add_junction_frames_batch_dev: the database is full (max_frames)");
  hipStream_t st = stream_of(c, stream);
  const int first = db->size;
  // map_refiner.cc:986-994: FrameToBow + AddFrame per keyframe; frame.cc:581-629 for the same frames
  if (bow_vector_queue(c, d_junc, d_njunc, B, capJ, db->j_ids, db->j_vals, db->j_nw, db->j_qword, st)) return 1;
  if (bowdb_add_impl(db, db->j_ids, db->j_vals, db->j_nw, d_junc, d_njunc, B, capJ, hipMemcpyDeviceToDevice, st, "bowdb_add_junction_frames_batch_dev")) return 1;
  if (junction_connect_queue(c, d_lines, d_nlines, capL, d_junc, d_njunc, capJ, B, W, H, db->j_edge, db->j_ecap, db->j_nedge, db->j_qstatus, nullptr, st))
    return 1;
  return junction_keys_queue(db, db->j_frames, first, B, db->j_qword, d_njunc, db->j_edge, db->j_nedge, db->j_qstatus, db->j_word, db->j_nj, st);
} AIRFE_CATCH(db->c)

}  // extern "C"
