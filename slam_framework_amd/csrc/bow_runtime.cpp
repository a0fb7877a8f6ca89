// bow_runtime.cpp -- host side of include/slamgpu_bow.h: vocabulary loading and its device
// layout, the synchronous per-frame calls (staged through the calling thread's buffer and stream,
// host_stage.h) and the batched *_device calls (validate, launch on the caller's stream, never
// allocate).
#include <hip/hip_runtime.h>

#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/slamgpu_bow.h"
#include "bow_kernels.h"
#include "host_stage.h"
#include "kfdb_kernels.h"
#include "stage_layout.h"

using namespace slamgpu;

static_assert(sizeof(slamgpu_bow_vec_view) == sizeof(BowVecView), "slamgpu_bow_vec_view layout");
static_assert(sizeof(slamgpu_bow_view) == sizeof(BowView), "slamgpu_bow_view layout");
static_assert(sizeof(slamgpu_keypoint) == sizeof(KeyPoint), "keypoint layout");

struct slamgpu_vocab {
  int device = 0;
  int k = 0, L = 0, scoring = 0, weighting = 0, n_words = 0;
  std::vector<int32_t> parent;
  std::vector<uint8_t> leaf, desc;
  std::vector<double> weight;
  uint4* d_slot_desc = nullptr;
  VocabSlot* d_slot = nullptr;
  uint32_t* d_node_word = nullptr;
  double* d_node_weight = nullptr;
  uint32_t root_first = 0, root_count = 0;
};

namespace {

void release(slamgpu_vocab* v) {
  if (!v) return;
  (void)hipSetDevice(v->device);
  if (v->d_slot_desc) (void)hipFree(v->d_slot_desc);
  if (v->d_slot) (void)hipFree(v->d_slot);
  if (v->d_node_word) (void)hipFree(v->d_node_word);
  if (v->d_node_weight) (void)hipFree(v->d_node_weight);
  delete v;
}

// Device layout: the children of every node, in file order, are contiguous slots (slot s = entry
// s of the parent-grouped child list), so one descent level reads one contiguous run of slots.
int upload(slamgpu_vocab* v) {
  const int n = (int)v->parent.size();
  std::vector<int32_t> cstart(n + 1, 0), child(n > 1 ? n - 1 : 1, 0);
  for (int i = 1; i < n; i++) cstart[v->parent[i] + 1]++;
  for (int i = 0; i < n; i++) cstart[i + 1] += cstart[i];
  std::vector<int32_t> fill(cstart.begin(), cstart.end() - 1);
  for (int i = 1; i < n; i++) child[fill[v->parent[i]]++] = i;
  const int ns = n > 1 ? n - 1 : 1;
  std::vector<uint8_t> sdesc((size_t)ns * 32, 0);
  std::vector<VocabSlot> slot(ns, VocabSlot{0, 0, 0, 0});
  for (int s = 0; s < n - 1; s++) {
    const int node = child[s];
    std::memcpy(&sdesc[(size_t)s * 32], &v->desc[(size_t)node * 32], 32);
    const int cnt = cstart[node + 1] - cstart[node];
    if (cnt > 0xffff) return t_bow_err.fail(SLAMGPU_EINVAL, "node %d has %d children (max 65535)", node, cnt);
    slot[s] = VocabSlot{(uint32_t)node, (uint32_t)cstart[node], (uint32_t)cnt, 0u};
  }
  if (cstart[1] > 0xffff) return t_bow_err.fail(SLAMGPU_EINVAL, "the root has %d children (max 65535)", cstart[1]);
  v->root_first = 0;
  v->root_count = (uint32_t)cstart[1];
  std::vector<uint32_t> word(n, 0);
  int words = 0;
  for (int i = 1; i < n; i++)
    if (v->leaf[i]) word[i] = (uint32_t)words++;  // TemplatedVocabulary.h:1405-1412
  v->n_words = words;
  HIPCHECK(t_bow_err, hipSetDevice(v->device));
  HIPCHECK(t_bow_err, hipMalloc(&v->d_slot_desc, sdesc.size()));
  HIPCHECK(t_bow_err, hipMalloc(&v->d_slot, sizeof(VocabSlot) * slot.size()));
  HIPCHECK(t_bow_err, hipMalloc(&v->d_node_word, sizeof(uint32_t) * n));
  HIPCHECK(t_bow_err, hipMalloc(&v->d_node_weight, sizeof(double) * n));
  HIPCHECK(t_bow_err, hipMemcpy(v->d_slot_desc, sdesc.data(), sdesc.size(), hipMemcpyHostToDevice));
  HIPCHECK(t_bow_err, hipMemcpy(v->d_slot, slot.data(), sizeof(VocabSlot) * slot.size(),
                         hipMemcpyHostToDevice));
  HIPCHECK(t_bow_err, hipMemcpy(v->d_node_word, word.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
  HIPCHECK(t_bow_err, hipMemcpy(v->d_node_weight, v->weight.data(), sizeof(double) * n,
                         hipMemcpyHostToDevice));
  return 0;
}

VocabDev device_view(const slamgpu_vocab* v, int levelsup) {
  VocabDev d;
  d.slot_desc = v->d_slot_desc;
  d.slot = v->d_slot;
  d.node_word = v->d_node_word;
  d.node_weight = v->d_node_weight;
  d.root_first = v->root_first;
  d.root_count = v->root_count;
  d.nid_level = v->L - levelsup;
  d.empty = (v->n_words == 0 || v->root_count == 0) ? 1 : 0;  // empty() (:1131)
  d.must = v->scoring != SLAMGPU_DOT_PRODUCT;  // ScoringObject.h:74-89
  d.l2 = v->scoring == SLAMGPU_L2_NORM;
  d.tf = (v->weighting == SLAMGPU_TF_IDF || v->weighting == SLAMGPU_TF) ? 1 : 0;
  return d;
}

int check_header(int k, int L, int scoring, int weighting) {
  // loadFromTextFile's header check (TemplatedVocabulary.h:1356-1360)
  if (k < 0 || k > 20 || L < 1 || L > 10 || scoring < 0 || scoring > 5 || weighting < 0 ||
      weighting > 3)
    return t_bow_err.fail(SLAMGPU_EINVAL,
                "Vocabulary loading failure: not a correct vocabulary (k %d, L %d, scoring %d, "
                "weighting %d)", k, L, scoring, weighting);
  return 0;
}

slamgpu_vocab* new_vocab(int device, int k, int L, int scoring, int weighting) {
  slamgpu_vocab* v = new slamgpu_vocab();
  v->device = device;
  v->k = k;
  v->L = L;
  v->scoring = scoring;
  v->weighting = weighting;
  v->parent.assign(1, 0);  // node 0 = the root (:1373-1374)
  v->leaf.assign(1, 0);
  v->desc.assign(32, 0);
  v->weight.assign(1, 0.0);
  return v;
}

int finish(slamgpu_vocab* v, slamgpu_vocab** out) {
  if (int r = upload(v)) {
    release(v);
    return r;
  }
  *out = v;
  return 0;
}

// A host FeatureVector must be well formed before its indices reach the device.
int check_set(const slamgpu_bow_set* s, const char* name) {
  if (!s) return t_bow_err.fail(SLAMGPU_EINVAL, "%s is NULL", name);
  if (s->n < 0 || s->n > SLAMGPU_BOW_MAX_FEATURES)
    return t_bow_err.fail(SLAMGPU_EINVAL, "%s: n %d outside [0, %d]", name, s->n, SLAMGPU_BOW_MAX_FEATURES);
  if (s->n_nodes < 0 || s->n_nodes > s->n)
    return t_bow_err.fail(SLAMGPU_EINVAL, "%s: n_nodes %d outside [0, n]", name, s->n_nodes);
  if (s->n > 0 && (!s->desc || !s->kps)) return t_bow_err.fail(SLAMGPU_EINVAL, "%s: NULL desc/kps", name);
  if (s->n_nodes > 0)
    return check_feature_vector(t_bow_err, name, s->n, s->n_nodes, s->nodes, s->node_start,
                                s->node_feats, "%s: feature index %u >= n");
  return 0;
}

}  // namespace

extern "C" {

const char* slamgpu_bow_last_error(void) { return t_bow_err.c_str(); }

int slamgpu_vocab_create(int device, int k, int L, int scoring, int weighting, int n_nodes,
                         const int32_t* parent, const uint8_t* leaf, const uint8_t* desc,
                         const double* weight, slamgpu_vocab** out) {
  if (!out) return t_bow_err.fail(SLAMGPU_EINVAL, "out is NULL");
  *out = nullptr;
  if (int r = check_header(k, L, scoring, weighting)) return r;
  if (n_nodes < 1) return t_bow_err.fail(SLAMGPU_EINVAL, "n_nodes %d < 1 (the root)", n_nodes);
  if (n_nodes > 1 && (!parent || !leaf || !desc || !weight))
    return t_bow_err.fail(SLAMGPU_EINVAL, "NULL node array");
  for (int i = 1; i < n_nodes; i++)
    if (parent[i] < 0 || parent[i] >= i)
      return t_bow_err.fail(SLAMGPU_EINVAL, "node %d: parent %d is not an earlier node", i, parent[i]);
  slamgpu_vocab* v = new_vocab(device, k, L, scoring, weighting);
  for (int i = 1; i < n_nodes; i++) {
    v->parent.push_back(parent[i]);
    v->leaf.push_back(leaf[i] ? 1 : 0);
    v->desc.insert(v->desc.end(), desc + (size_t)i * 32, desc + (size_t)i * 32 + 32);
    v->weight.push_back(weight[i]);
  }
  return finish(v, out);
}

int slamgpu_vocab_load_text(int device, const char* path, slamgpu_vocab** out) {
  if (!out || !path) return t_bow_err.fail(SLAMGPU_EINVAL, "NULL argument");
  *out = nullptr;
  std::ifstream f(path);
  if (!f.is_open()) return t_bow_err.fail(SLAMGPU_EINVAL, "cannot open %s", path);
  std::string s;
  std::getline(f, s);
  std::stringstream ss(s);
  int k = -1, L = -1, n1 = -1, n2 = -1;
  ss >> k >> L >> n1 >> n2;
  if (int r = check_header(k, L, n1, n2)) return r;
  slamgpu_vocab* v = new_vocab(device, k, L, n1, n2);
  std::string line;
  while (std::getline(f, line)) {
    if (line.find_first_not_of(" \t\r") == std::string::npos) continue;  // declared: no node
    std::stringstream ls(line);
    int pid = 0, is_leaf = 0;
    ls >> pid >> is_leaf;
    // the 32 descriptor fields are read as strings and re-parsed (F::fromString, FORB.cpp:120)
    std::stringstream ssd;
    for (int i = 0; i < 32; i++) {
      std::string e;
      ls >> e;
      ssd << e << " ";
    }
    uint8_t d[32] = {0};
    for (int i = 0; i < 32; i++) {
      int x = 0;
      ssd >> x;
      if (!ssd.fail()) d[i] = (uint8_t)x;
    }
    double w = 0.0;
    ls >> w;
    const int nid = (int)v->parent.size();
    if (pid < 0 || pid >= nid) {
      release(v);
      return t_bow_err.fail(SLAMGPU_EINVAL, "%s: node %d names parent %d", path, nid, pid);
    }
    v->parent.push_back(pid);
    v->leaf.push_back(is_leaf > 0 ? 1 : 0);
    v->desc.insert(v->desc.end(), d, d + 32);
    v->weight.push_back(w);
  }
  return finish(v, out);
}

void slamgpu_vocab_destroy(slamgpu_vocab* v) { release(v); }

int slamgpu_vocab_info(const slamgpu_vocab* v, int32_t* info) {
  if (!v || !info) return t_bow_err.fail(SLAMGPU_EINVAL, "NULL argument");
  info[0] = v->k;
  info[1] = v->L;
  info[2] = v->scoring;
  info[3] = v->weighting;
  info[4] = (int32_t)v->parent.size();
  info[5] = v->n_words;
  return 0;
}

int slamgpu_vocab_nodes(const slamgpu_vocab* v, int32_t* parent, uint8_t* leaf, uint8_t* desc,
                        double* weight) {
  if (!v) return t_bow_err.fail(SLAMGPU_EINVAL, "NULL vocabulary");
  const size_t n = v->parent.size();
  if (parent) std::memcpy(parent, v->parent.data(), n * sizeof(int32_t));
  if (leaf) std::memcpy(leaf, v->leaf.data(), n);
  if (desc) std::memcpy(desc, v->desc.data(), n * 32);
  if (weight) std::memcpy(weight, v->weight.data(), n * sizeof(double));
  return 0;
}

int slamgpu_bow_transform_device(slamgpu_vocab* v, const uint8_t* d_desc, int64_t set_stride,
                                 const int32_t* d_counts, int count_step, int n_sets,
                                 int levelsup, const slamgpu_bow_sets* out, void* stream) {
  if (!v || !out) return t_bow_err.fail(SLAMGPU_EINVAL, "NULL argument");
  if (n_sets < 0 || n_sets > 65535) return t_bow_err.fail(SLAMGPU_EINVAL, "n_sets %d outside [0, 65535]", n_sets);
  if (n_sets == 0) return 0;
  if (out->cap < 1 || out->cap > SLAMGPU_BOW_MAX_FEATURES)
    return t_bow_err.fail(SLAMGPU_EINVAL, "cap %d outside [1, %d]", out->cap, SLAMGPU_BOW_MAX_FEATURES);
  if (count_step < 1 || set_stride < 0) return t_bow_err.fail(SLAMGPU_EINVAL, "bad set_stride/count_step");
  if (!d_desc || !d_counts || !out->words || !out->values || !out->n_words || !out->nodes ||
      !out->node_start || !out->node_feats || !out->n_nodes || !out->feat_leaf || !out->feat_node)
    return t_bow_err.fail(SLAMGPU_EINVAL, "NULL device buffer");
  HIPCHECK(t_bow_err, hipSetDevice(v->device));
  const BowSets o{out->words, out->values, out->n_words, out->nodes, out->node_start,
                  out->node_feats, out->n_nodes, out->feat_leaf, out->feat_node, out->cap};
  HIPCHECK(t_bow_err, launch_bow_transform(device_view(v, levelsup), d_desc, set_stride, d_counts,
                                    count_step, n_sets, o, static_cast<hipStream_t>(stream)));
  return 0;
}

int slamgpu_bow_transform(slamgpu_vocab* v, const uint8_t* desc, int n, int levelsup,
                          uint32_t* words, double* values, int* n_words, uint32_t* nodes,
                          int32_t* node_start, uint32_t* node_feats, int* n_nodes) {
  if (!v || !n_words || !n_nodes || !node_start) return t_bow_err.fail(SLAMGPU_EINVAL, "NULL argument");
  if (n < 0 || n > SLAMGPU_BOW_MAX_FEATURES)
    return t_bow_err.fail(SLAMGPU_ECAP, "n %d outside [0, %d]", n, SLAMGPU_BOW_MAX_FEATURES);
  if (n > 0 && (!desc || !words || !values || !nodes || !node_feats))
    return t_bow_err.fail(SLAMGPU_EINVAL, "NULL buffer");
  const int cap = n > 0 ? n : 1;
  HIPCHECK(t_bow_err, hipSetDevice(v->device));
  StageLease S(t_bow_err);
  StageLayout L;
  const BowTransformLayout t = layout_bow_transform(L, cap);
  if (int r = S.reserve(L.size())) return r;
  hipStream_t st = S.stream();
  const int32_t cnt = n;
  HIPCHECK(t_bow_err, S.upload(t.desc, desc, (size_t)n * 32));
  HIPCHECK(t_bow_err, S.upload(t.cnt, &cnt, 4));
  const BowSets o{S.at<uint32_t>(t.words), S.at<double>(t.values), S.at<int32_t>(t.n_words),
                  S.at<uint32_t>(t.nodes), S.at<int32_t>(t.node_start), S.at<uint32_t>(t.node_feats),
                  S.at<int32_t>(t.n_nodes), S.at<uint32_t>(t.feat_leaf),
                  S.at<uint32_t>(t.feat_node), cap};
  HIPCHECK(t_bow_err, launch_bow_transform(device_view(v, levelsup), S.at<uint8_t>(t.desc), 0,
                                                   S.at<int32_t>(t.cnt), 1, 1, o, st));
  int32_t nw = 0, nn = 0;
  HIPCHECK(t_bow_err, S.download(&nw, t.n_words, 4));
  HIPCHECK(t_bow_err, S.download(&nn, t.n_nodes, 4));
  HIPCHECK(t_bow_err, hipStreamSynchronize(st));
  HIPCHECK(t_bow_err, S.download(words, t.words, (size_t)nw * 4));
  HIPCHECK(t_bow_err, S.download(values, t.values, (size_t)nw * 8));
  HIPCHECK(t_bow_err, S.download(node_start, t.node_start, (size_t)(nn + 1) * 4));
  HIPCHECK(t_bow_err, S.download(nodes, t.nodes, (size_t)nn * 4));
  HIPCHECK(t_bow_err, hipStreamSynchronize(st));
  if (nn > 0)
    HIPCHECK(t_bow_err, S.download(node_feats, t.node_feats, (size_t)node_start[nn] * 4));
  HIPCHECK(t_bow_err, hipStreamSynchronize(st));
  *n_words = nw;
  *n_nodes = nn;
  return 0;
}

// Only L1Scoring is built; the message names what the vocabulary asks for.
static int check_scoring(const slamgpu_vocab* v) {
  static const char* const names[6] = {"L1_NORM", "L2_NORM", "CHI_SQUARE", "KL", "BHATTACHARYYA",
                                       "DOT_PRODUCT"};
  if (!v) return t_bow_err.fail(SLAMGPU_EINVAL, "NULL vocabulary");
  if (v->scoring != SLAMGPU_L1_NORM)
    return t_bow_err.fail(SLAMGPU_EINVAL, "score: the vocabulary's scoring %s is not built (only L1_NORM)",
                          names[v->scoring]);
  return 0;
}

int slamgpu_bow_score_device(const slamgpu_vocab* v, const slamgpu_bow_vec_view* d_a,
                             const slamgpu_bow_vec_view* d_b, int n_pairs, double* d_scores,
                             void* stream) {
  if (int r = check_scoring(v)) return r;
  if (n_pairs < 0) return t_bow_err.fail(SLAMGPU_EINVAL, "n_pairs %d < 0", n_pairs);
  if (n_pairs == 0) return 0;
  if (!d_a || !d_b || !d_scores) return t_bow_err.fail(SLAMGPU_EINVAL, "NULL device buffer");
  HIPCHECK(t_bow_err, hipSetDevice(v->device));
  HIPCHECK(t_bow_err, launch_bow_score(reinterpret_cast<const BowVecView*>(d_a),
                                       reinterpret_cast<const BowVecView*>(d_b), n_pairs, d_scores,
                                       static_cast<hipStream_t>(stream)));
  return 0;
}

int slamgpu_bow_score(const slamgpu_vocab* v, const slamgpu_bow_vec* a, const slamgpu_bow_vec* b,
                      int n_pairs, double* scores) {
  if (int r = check_scoring(v)) return r;
  if (n_pairs < 0) return t_bow_err.fail(SLAMGPU_EINVAL, "n_pairs %d < 0", n_pairs);
  if (n_pairs == 0) return 0;
  if (!a || !b || !scores) return t_bow_err.fail(SLAMGPU_EINVAL, "NULL argument");
  size_t total = 0;
  for (int p = 0; p < n_pairs; p++)
    for (const slamgpu_bow_vec* s : {&a[p], &b[p]}) {
      if (s->n < 0 || (s->n > 0 && (!s->words || !s->values)))
        return t_bow_err.fail(SLAMGPU_EINVAL, "pair %d: bad BowVector (n %d)", p, s->n);
      for (int i = 1; i < s->n; i++)
        if (s->words[i] <= s->words[i - 1])
          return t_bow_err.fail(SLAMGPU_EINVAL, "pair %d: words not strictly ascending", p);
      total += (size_t)s->n;
    }
  HIPCHECK(t_bow_err, hipSetDevice(v->device));
  StageLease S(t_bow_err);
  StageLayout L;
  const BowScoreLayout l = layout_bow_score(L, n_pairs, total);
  if (int r = S.reserve(L.size())) return r;
  // views[p] = a[p], views[n_pairs + p] = b[p]
  std::vector<slamgpu_bow_vec_view> views(2 * (size_t)n_pairs);
  std::vector<int32_t> counts(2 * (size_t)n_pairs);
  size_t at = 0;
  for (int side = 0; side < 2; side++)
    for (int p = 0; p < n_pairs; p++) {
      const slamgpu_bow_vec& s = side ? b[p] : a[p];
      const size_t k = (size_t)side * n_pairs + p;
      HIPCHECK(t_bow_err, S.upload(l.words + at * 4, s.words, (size_t)s.n * 4));
      HIPCHECK(t_bow_err, S.upload(l.values + at * 8, s.values, (size_t)s.n * 8));
      counts[k] = s.n;
      views[k] = {S.at<uint32_t>(l.words) + at, S.at<double>(l.values) + at,
                  S.at<int32_t>(l.counts) + k};
      at += (size_t)s.n;
    }
  HIPCHECK(t_bow_err, S.upload(l.counts, counts.data(), counts.size() * 4));
  HIPCHECK(t_bow_err, S.upload(l.views, views.data(), views.size() * sizeof(views[0])));
  const BowVecView* dv = S.at<BowVecView>(l.views);
  HIPCHECK(t_bow_err, launch_bow_score(dv, dv + n_pairs, n_pairs, S.at<double>(l.scores), S.stream()));
  HIPCHECK(t_bow_err, S.download(scores, l.scores, (size_t)n_pairs * 8));
  HIPCHECK(t_bow_err, hipStreamSynchronize(S.stream()));
  return 0;
}

int slamgpu_search_by_bow_device(const slamgpu_bow_view* d_a, const slamgpu_bow_view* d_b,
                                 int n_pairs, int kf_kf, float nnratio, int check_ori,
                                 int32_t* d_match, int64_t match_stride, int32_t* d_nmatches,
                                 void* stream) {
  if (n_pairs < 0) return t_bow_err.fail(SLAMGPU_EINVAL, "n_pairs %d < 0", n_pairs);
  if (n_pairs == 0) return 0;
  if (!d_a || !d_b || !d_match || !d_nmatches) return t_bow_err.fail(SLAMGPU_EINVAL, "NULL device buffer");
  if (match_stride < 0) return t_bow_err.fail(SLAMGPU_EINVAL, "match_stride < 0");
  HIPCHECK(t_bow_err, launch_search_bow(reinterpret_cast<const BowView*>(d_a),
                                 reinterpret_cast<const BowView*>(d_b), n_pairs, kf_kf ? 1 : 0,
                                 nnratio, check_ori ? 1 : 0, d_match, match_stride, d_nmatches,
                                 static_cast<hipStream_t>(stream)));
  return 0;
}

int slamgpu_search_by_bow(const slamgpu_bow_set* a, const slamgpu_bow_set* b, int kf_kf,
                          float nnratio, int check_ori, int32_t* match_a, int* nmatches) {
  if (int r = check_set(a, "a")) return r;
  if (int r = check_set(b, "b")) return r;
  if (!nmatches || (a->n > 0 && !match_a)) return t_bow_err.fail(SLAMGPU_EINVAL, "NULL output");
  const uint8_t* b_valid = kf_kf ? b->valid : nullptr;
  StageLease S(t_bow_err);
  StageLayout L;
  const BowSearchLayout l = layout_search_by_bow(L, a->n, a->n_nodes, b->n, b->n_nodes);
  if (int r = S.reserve(L.size())) return r;
  hipStream_t st = S.stream();
  slamgpu_bow_view views[2];
  auto upload_set = [&](const slamgpu_bow_set* s, const BowSetPlace& p, const uint8_t* valid,
                        slamgpu_bow_view* vw) -> int {
    const int32_t cnt[2] = {s->n, s->n_nodes};
    HIPCHECK(t_bow_err, S.upload(p.desc, s->desc, (size_t)s->n * 32));
    HIPCHECK(t_bow_err, S.upload(p.kps, s->kps, (size_t)s->n * sizeof(slamgpu_keypoint)));
    HIPCHECK(t_bow_err, S.upload(p.valid, valid, (size_t)s->n));
    HIPCHECK(t_bow_err, S.upload(p.cnt, cnt, 8));
    if (s->n_nodes > 0) {
      HIPCHECK(t_bow_err, S.upload(p.nodes, s->nodes, (size_t)s->n_nodes * 4));
      HIPCHECK(t_bow_err, S.upload(p.node_start, s->node_start, (size_t)(s->n_nodes + 1) * 4));
      HIPCHECK(t_bow_err, S.upload(p.node_feats, s->node_feats,
                                           (size_t)s->node_start[s->n_nodes] * 4));
    }
    vw->desc = S.at<uint8_t>(p.desc);
    vw->kps = S.at<slamgpu_keypoint>(p.kps);
    vw->valid = valid ? S.at<uint8_t>(p.valid) : nullptr;
    vw->n = S.at<int32_t>(p.cnt);
    vw->n_nodes = S.at<int32_t>(p.cnt) + 1;
    vw->nodes = S.at<uint32_t>(p.nodes);
    vw->node_start = S.at<int32_t>(p.node_start);
    vw->node_feats = S.at<uint32_t>(p.node_feats);
    return 0;
  };
  // the pair's hipMemcpyAsync sources must outlive the copies: synchronise before returning
  if (int r = upload_set(a, l.a, a->valid, &views[0])) return r;
  if (int r = upload_set(b, l.b, b_valid, &views[1])) return r;
  HIPCHECK(t_bow_err, S.upload(l.views, views, sizeof(views)));
  const BowView* dv = S.at<BowView>(l.views);
  HIPCHECK(t_bow_err, launch_search_bow(dv, dv + 1, 1, kf_kf ? 1 : 0, nnratio,
                                                check_ori ? 1 : 0, S.at<int32_t>(l.match), 0,
                                                S.at<int32_t>(l.nmatches), st));
  int32_t nm = 0;
  HIPCHECK(t_bow_err, S.download(&nm, l.nmatches, 4));
  HIPCHECK(t_bow_err, S.download(match_a, l.match, (size_t)a->n * 4));
  HIPCHECK(t_bow_err, hipStreamSynchronize(st));
  *nmatches = nm;
  return 0;
}

int slamgpu_distinctive_descriptors_device(const uint8_t* d_desc, const int32_t* d_start,
                                           int n_points, int32_t* d_best, uint8_t* d_desc_out,
                                           void* stream) {
  if (n_points < 0) return t_bow_err.fail(SLAMGPU_EINVAL, "n_points %d < 0", n_points);
  if (n_points == 0) return 0;
  if (!d_desc || !d_start || !d_best) return t_bow_err.fail(SLAMGPU_EINVAL, "NULL device buffer");
  HIPCHECK(t_bow_err, launch_distinctive(d_desc, d_start, n_points, d_best, d_desc_out,
                                  static_cast<hipStream_t>(stream)));
  return 0;
}

int slamgpu_distinctive_descriptors(const uint8_t* desc, const int32_t* start, int n_points,
                                    int32_t* best, uint8_t* desc_out) {
  if (n_points < 0 || !start || (n_points > 0 && !best))
    return t_bow_err.fail(SLAMGPU_EINVAL, "bad arguments");
  if (n_points == 0) return 0;
  const int32_t s0 = start[0];
  for (int p = 0; p < n_points; p++)
    if (start[p + 1] < start[p] || start[p + 1] - start[p] > 65535 || start[p] < 0)
      return t_bow_err.fail(SLAMGPU_EINVAL, "start not ascending (or a point with > 65535 descriptors)");
  const int total = start[n_points] - s0;
  if (total > 0 && !desc) return t_bow_err.fail(SLAMGPU_EINVAL, "NULL desc");
  StageLease S(t_bow_err);
  StageLayout L;
  const DistinctiveLayout l = layout_distinctive(L, n_points, total);
  if (int r = S.reserve(L.size())) return r;
  hipStream_t st = S.stream();
  std::vector<int32_t> rel(n_points + 1);
  for (int p = 0; p <= n_points; p++) rel[p] = start[p] - s0;
  if (total > 0)
    HIPCHECK(t_bow_err, S.upload(l.desc, desc + (size_t)s0 * 32, (size_t)total * 32));
  HIPCHECK(t_bow_err, S.upload(l.start, rel.data(), rel.size() * 4));
  HIPCHECK(t_bow_err, launch_distinctive(S.at<uint8_t>(l.desc), S.at<int32_t>(l.start),
                                                 n_points, S.at<int32_t>(l.best),
                                                 desc_out ? S.at<uint8_t>(l.out) : nullptr, st));
  HIPCHECK(t_bow_err, S.download(best, l.best, (size_t)n_points * 4));
  HIPCHECK(t_bow_err, hipStreamSynchronize(st));
  if (desc_out) {
    std::vector<uint8_t> tmp((size_t)n_points * 32);
    HIPCHECK(t_bow_err, S.download(tmp.data(), l.out, tmp.size()));
    HIPCHECK(t_bow_err, hipStreamSynchronize(st));
    for (int p = 0; p < n_points; p++)
      if (best[p] >= 0) std::memcpy(desc_out + (size_t)p * 32, &tmp[(size_t)p * 32], 32);
  }
  return 0;
}

int slamgpu_gray_device(const uint8_t* d_src, size_t src_pitch, size_t src_stride, int channels,
                        int rgb, int cols, int rows, int n_images, uint8_t* d_dst,
                        size_t dst_pitch, size_t dst_stride, void* stream) {
  if (channels != 3 && channels != 4) return t_bow_err.fail(SLAMGPU_EINVAL, "channels %d not 3 or 4", channels);
  if (cols < 0 || rows < 0 || n_images < 0 || rows > 65535 || n_images > 65535)
    return t_bow_err.fail(SLAMGPU_EINVAL, "bad image geometry");
  if (src_pitch < (size_t)cols * channels || dst_pitch < (size_t)cols)
    return t_bow_err.fail(SLAMGPU_EINVAL, "pitch smaller than a row");
  if ((size_t)cols * rows * n_images > 0 && (!d_src || !d_dst))
    return t_bow_err.fail(SLAMGPU_EINVAL, "NULL device buffer");
  HIPCHECK(t_bow_err, launch_gray(d_src, src_pitch, src_stride, channels, rgb, cols, rows, n_images,
                           d_dst, dst_pitch, dst_stride, static_cast<hipStream_t>(stream)));
  return 0;
}

int slamgpu_gray(const uint8_t* src, size_t src_pitch, int channels, int rgb, int cols, int rows,
                 uint8_t* dst, size_t dst_pitch) {
  if (channels != 3 && channels != 4) return t_bow_err.fail(SLAMGPU_EINVAL, "channels %d not 3 or 4", channels);
  if (cols < 0 || rows < 0 || rows > 65535) return t_bow_err.fail(SLAMGPU_EINVAL, "bad image geometry");
  if (cols == 0 || rows == 0) return 0;
  if (!src || !dst || src_pitch < (size_t)cols * channels || dst_pitch < (size_t)cols)
    return t_bow_err.fail(SLAMGPU_EINVAL, "bad buffers");
  const size_t sp = (size_t)cols * channels, dp = (size_t)cols;
  StageLease S(t_bow_err);
  StageLayout L;
  const GrayLayout g = layout_gray(L, sp * rows, dp * rows);
  if (int r = S.reserve(L.size())) return r;
  hipStream_t st = S.stream();
  uint8_t* d_src = S.at<uint8_t>(g.src);
  uint8_t* d_dst = S.at<uint8_t>(g.dst);
  HIPCHECK(t_bow_err, hipMemcpy2DAsync(d_src, sp, src, src_pitch, sp, rows,
                                               hipMemcpyHostToDevice, st));
  HIPCHECK(t_bow_err, launch_gray(d_src, sp, 0, channels, rgb, cols, rows, 1, d_dst, dp, 0, st));
  HIPCHECK(t_bow_err, hipMemcpy2DAsync(dst, dst_pitch, d_dst, dp, dp, rows,
                                               hipMemcpyDeviceToHost, st));
  HIPCHECK(t_bow_err, hipStreamSynchronize(st));
  return 0;
}

}  // extern "C"
