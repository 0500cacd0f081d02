/*
 * map_oracle.c -- CPU ORACLE for the mapper's map.  TEST INFRASTRUCTURE ONLY (see icp_oracle.h:
 * PARITY UNPINNED -- the octree is PCL's, which is not under /root/reference).
 *
 * Restates what the reference relies on at
 *   /root/reference/src/icpslam/octree_mapper.cpp:55-59   resetMap (OctreePointCloudSearch, resolution 0.5 m)
 *   /root/reference/src/icpslam/octree_mapper.cpp:62-69   addPointsToMap: "if (!isVoxelOccupiedAtPoint(p)) addPointToCloud(p)"
 *   /root/reference/src/icpslam/octree_mapper.cpp:72-90   approxNearestNeighbors -> nn cloud
 * as a plain sequential loop: points are visited in order; a point is appended iff its voxel is empty; the voxel is PCL's
 * genOctreeKeyforPoint, trunc((p - min) / resolution) in double under the octree's bounding box IN FORCE WHEN THE POINT IS
 * TESTED (PCL OctreePointCloud::adoptBoundingBoxToPoint sets the first box to p +- resolution / 2 and calls getKeyBitSize(),
 * which -- max_voxels = max(ceil(extent / resolution), 2) -- makes the tree one level deep, 2 voxels wide: p +- resolution;
 * every point outside the box doubles it towards that point and is appended whatever its voxel holds, isVoxelOccupiedAtPoint
 * being false outside the box).  The minimum moves by whole side lengths, but each move rounds in double: for a resolution
 * that is not a power of two a point on a voxel face can key one voxel off floor((p - first minimum) / resolution), the fixed
 * lattice this file used until the face campaign of tests/test_map_oracle.py found the difference (powers of two round
 * exactly and were never affected).  The nearest-neighbour query is EXACT (orc_nn), where PCL's approxNearestSearch is a
 * heuristic descent -- SURVEY.md 8(f4) asks for the exact one; orc_octree_* at the end of this file restate PCL's tree and
 * approxNearestSearch themselves.
 *
 * The voxel set is a sorted array + binary search: deliberately nothing like the GPU's hash set.  Two forms of addPointsToMap:
 * orc_map_add_points_sequential is the reference's loop as written (one point at a time, O(map) per insertion: fine to ~100k
 * map points); orc_map_add_points states the same rule per batch -- a point is appended iff its voxel is not in the map before
 * the call AND no earlier point of the call has it -- with one sort of the batch's (voxel, index) pairs, so that a 1M-point map
 * (BASELINE config 3's scale) takes seconds.  tests/test_map_oracle.py holds the two against each other.
 */
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "icp_oracle.h"

/* ---- PCL 1.8's OctreePointCloud bounding box (octree_pointcloud.hpp), operation for operation, in double ---------------- */
#define ORC_KEY_REACH ((1ll << 20) - 1) /* voxels either side of the first box's minimum a map key may lie (21 bits per axis) */
#define ORC_FAR (1048576.0 + 2.0)      /* beyond this many voxels from the first box a point cannot be in reach: not looked at */

typedef struct {
  int defined, depth;    /* depth: levels below the root, side = 2^depth voxels */
  double min[3], max[3]; /* min_x_ .. max_z_ */
  long long shift[3];    /* whole voxels the minimum has moved since the first box */
  double origin[3];      /* the first box's minimum */
} orc_box;

static const double kMinValue = (double)FLT_EPSILON; /* PCL: const float minValue = std::numeric_limits<float>::epsilon() */

/* getKeyBitSize() on an octree without leaves: max_voxels = max(ceil(extent / res), 2), the oversize split evenly */
static void box_key_bit_size(orc_box* b, double res) {
  unsigned int max_key = 0;
  for (int a = 0; a < 3; ++a) {
    const unsigned int k = (unsigned int)ceil((b->max[a] - b->min[a] - kMinValue) / res);
    if (k > max_key) max_key = k;
  }
  const unsigned int max_voxels = max_key > 2u ? max_key : 2u;
  b->depth = (int)(unsigned int)ceil(log((double)max_voxels) / log(2.0) - kMinValue);
  const double side = (double)(1u << b->depth) * res;
  for (int a = 0; a < 3; ++a) {
    const double oversize = (side - (b->max[a] - b->min[a])) / 2.0;
    if (oversize > kMinValue) {
      b->min[a] -= oversize;
      b->max[a] += oversize;
    }
  }
}

/* isPointWithinBoundingBox */
static int box_inside(const orc_box* b, const float* p) {
  return b->defined && !((double)p[0] < b->min[0] || (double)p[1] < b->min[1] || (double)p[2] < b->min[2] ||
                         (double)p[0] >= b->max[0] || (double)p[1] >= b->max[1] || (double)p[2] >= b->max[2]);
}

/* one pass of adoptBoundingBoxToPoint's loop: 0 if p is inside the (defined) box; otherwise the box is defined (first point:
 * p +- res / 2, then getKeyBitSize) or doubled towards p, and *child is the old root's child index in the new root (-1 for
 * the first box) */
static int box_step(orc_box* b, const float* p, double res, int* child) {
  if (!b->defined) {
    for (int a = 0; a < 3; ++a) {
      b->min[a] = (double)p[a] - res / 2;
      b->max[a] = (double)p[a] + res / 2;
      b->shift[a] = 0;
    }
    box_key_bit_size(b, res);
    for (int a = 0; a < 3; ++a) b->origin[a] = b->min[a];
    b->defined = 1;
    *child = -1;
    return 1;
  }
  int up[3], any = 0;
  for (int a = 0; a < 3; ++a) {
    up[a] = (double)p[a] >= b->max[a];
    any |= up[a] || (double)p[a] < b->min[a];
  }
  if (!any) return 0;
  *child = (!up[0] << 2) | (!up[1] << 1) | !up[2]; /* the old root becomes the UPPER child where p is not above */
  const double side = (double)(1ll << b->depth) * res;
  for (int a = 0; a < 3; ++a)
    if (!up[a]) {
      b->min[a] -= side;
      b->shift[a] += 1ll << b->depth;
    }
  b->depth += 1;
  const double len = (double)(1ll << b->depth) * res - kMinValue;
  for (int a = 0; a < 3; ++a) b->max[a] = b->min[a] + len;
  return 1;
}

/* genOctreeKeyforPoint: static_cast<unsigned int>((p - min) / res) -- truncation -- under the box in force */
static void box_key(const orc_box* b, const float* p, double res, long long k[3]) {
  for (int a = 0; a < 3; ++a) k[a] = (long long)(((double)p[a] - b->min[a]) / res);
}

/* a point this far from the first box can never get a key in reach; it is not looked at (and never grows the box) */
static int box_far(const orc_box* b, const float* p, double res) {
  if (!b->defined) return 0;
  for (int a = 0; a < 3; ++a)
    if (!(fabs(((double)p[a] - b->origin[a]) / res) <= ORC_FAR)) return 1;
  return 0;
}

/* ---- the lattice form: a sorted array of voxel keys ------------------------------------------------------------------ */
struct orc_map {
  double res;
  orc_box box;
  size_t n, cap;
  float* pts;     /* n x 4 */
  int64_t* keys;  /* sorted voxel keys of the n points (a key may repeat: see map_candidate) */
};

static int64_t pack_key(int64_t kx, int64_t ky, int64_t kz) { return ((kz + (1 << 20)) << 42) | ((ky + (1 << 20)) << 21) | (kx + (1 << 20)); }

/* What addPointsToMap does with the finite point p, the box advanced as PCL advances it:
 *   0  dropped: non-finite, or its key (in the first box's frame) beyond +-ORC_KEY_REACH -- the box is left as it was;
 *   1  inside the box: appended iff no map point has *key (isVoxelOccupiedAtPoint);
 *   2  outside the box (or the first point): isVoxelOccupiedAtPoint is false, so it is appended whatever *key holds, and the
 *      box has grown to take it (adoptBoundingBoxToPoint); *key is its key under the grown box.
 * The key of a point is trunc((p - min_v) / res) - shift_v under the box v in force when it is tested: PCL's key, which for a
 * point on a voxel face can differ by one from floor((p - first box minimum) / res) once the minimum has moved (the moves
 * round in double; a power-of-two resolution rounds exactly). */
static int map_candidate(orc_box* box, double res, const float* p, int64_t* key) {
  if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) || box_far(box, p, res)) return 0;
  orc_box b = *box;
  const int inside = box_inside(&b, p);
  int child;
  while (box_step(&b, p, res, &child)) {
  }
  long long k[3];
  box_key(&b, p, res, k);
  for (int a = 0; a < 3; ++a) {
    k[a] -= b.shift[a];
    if (k[a] < -ORC_KEY_REACH || k[a] > ORC_KEY_REACH) return 0;
  }
  *key = pack_key(k[0], k[1], k[2]);
  if (inside) return 1;
  *box = b;
  return 2;
}

orc_map* orc_map_create(double resolution) {
  orc_map* m = (orc_map*)calloc(1, sizeof(orc_map));
  if (m) m->res = resolution;
  return m;
}

void orc_map_destroy(orc_map* m) {
  if (!m) return;
  free(m->pts);
  free(m->keys);
  free(m);
}

size_t orc_map_size(const orc_map* m) { return m->n; }
const float* orc_map_points(const orc_map* m) { return m->pts; }

static long find_key(const int64_t* keys, size_t n, int64_t k) { /* position of k in the sorted array or -(insert)-1 */
  size_t lo = 0, hi = n;
  while (lo < hi) {
    const size_t mid = (lo + hi) / 2;
    if (keys[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  return (lo < n && keys[lo] == k) ? (long)lo : -(long)lo - 1;
}

/* addPointsToMap(transformCloudToPoseFrame(cloud, pose)); returns the number of points appended, -1 on allocation failure */
long orc_map_add_points_sequential(orc_map* m, const float* in_xyzw, size_t n, const float pose[16]) {
  float* moved = (float*)malloc((n ? n : 1) * 4 * sizeof(float));
  if (!moved) return -1;
  if (pose) orc_transform_cloud(in_xyzw, n, pose, moved);
  else {
    memcpy(moved, in_xyzw, n * 4 * sizeof(float));
    for (size_t i = 0; i < n; ++i) moved[4 * i + 3] = 1.0f;
  }
  long added = 0;
  for (size_t i = 0; i < n; ++i) {
    const float* p = moved + 4 * i;
    int64_t key;
    const int c = map_candidate(&m->box, m->res, p, &key);
    if (!c) continue;
    const long pos = find_key(m->keys, m->n, key);
    if (c == 1 && pos >= 0) continue; /* isVoxelOccupiedAtPoint */
    if (m->n == m->cap) {
      const size_t cap = m->cap ? 2 * m->cap : 4096;
      float* np_ = (float*)realloc(m->pts, cap * 4 * sizeof(float));
      int64_t* nk = (int64_t*)realloc(m->keys, cap * sizeof(int64_t));
      if (np_) m->pts = np_;
      if (nk) m->keys = nk;
      if (!np_ || !nk) {
        free(moved);
        return -1;
      }
      m->cap = cap;
    }
    const size_t ins = pos >= 0 ? (size_t)pos : (size_t)(-pos - 1);
    memmove(m->keys + ins + 1, m->keys + ins, (m->n - ins) * sizeof(int64_t));
    m->keys[ins] = key;
    memcpy(m->pts + 4 * m->n, p, 4 * sizeof(float)); /* map_cloud_ keeps insertion order */
    m->n++;
    added++;
  }
  free(moved);
  return added;
}

/* the same rule, batch form (see the header comment) */
typedef struct { int64_t key; size_t i; int always; } orc_key_idx;
static int cmp_key_idx(const void* a, const void* b) {
  const orc_key_idx *x = (const orc_key_idx*)a, *y = (const orc_key_idx*)b;
  if (x->key != y->key) return x->key < y->key ? -1 : 1;
  return x->i < y->i ? -1 : (x->i > y->i ? 1 : 0);
}
static int cmp_size_t(const void* a, const void* b) {
  const size_t x = *(const size_t*)a, y = *(const size_t*)b;
  return x < y ? -1 : (x > y ? 1 : 0);
}

long orc_map_add_points(orc_map* m, const float* in_xyzw, size_t n, const float pose[16]) {
  float* moved = (float*)malloc((n ? n : 1) * 4 * sizeof(float));
  orc_key_idx* ki = (orc_key_idx*)malloc((n ? n : 1) * sizeof(orc_key_idx));
  size_t* first = (size_t*)malloc((n ? n : 1) * sizeof(size_t));
  if (!moved || !ki || !first) {
    free(moved);
    free(ki);
    free(first);
    return -1;
  }
  if (pose) orc_transform_cloud(in_xyzw, n, pose, moved);
  else {
    memcpy(moved, in_xyzw, n * 4 * sizeof(float));
    for (size_t i = 0; i < n; ++i) moved[4 * i + 3] = 1.0f;
  }
  size_t nk = 0;
  for (size_t i = 0; i < n; ++i) { /* the box is advanced in input order: every point is keyed under the box it is tested in */
    int64_t key;
    const int c = map_candidate(&m->box, m->res, moved + 4 * i, &key);
    if (!c) continue;
    ki[nk].key = key;
    ki[nk].i = i;
    ki[nk].always = c == 2;
    nk++;
  }
  qsort(ki, nk, sizeof(orc_key_idx), cmp_key_idx);
  /* per voxel, in input order: the first point if the map does not hold the voxel yet, and every point that grew the box */
  size_t nf = 0;
  int occupied = 0;
  for (size_t a = 0; a < nk; ++a) {
    if (!a || ki[a].key != ki[a - 1].key) occupied = find_key(m->keys, m->n, ki[a].key) >= 0; /* isVoxelOccupiedAtPoint */
    if (occupied && !ki[a].always) continue;
    occupied = 1;
    first[nf] = ki[a].i;
    ki[nf].key = ki[a].key; /* (nf <= a: the new points' keys, ascending, compacted to the front of ki) */
    nf++;
  }
  qsort(first, nf, sizeof(size_t), cmp_size_t); /* map_cloud_ keeps insertion order */
  const size_t total = m->n + nf;
  if (total > m->cap) {
    size_t cap = m->cap ? m->cap : 4096;
    while (cap < total) cap *= 2;
    float* np_ = (float*)realloc(m->pts, cap * 4 * sizeof(float));
    if (np_) m->pts = np_;
    int64_t* nkeys = (int64_t*)realloc(m->keys, cap * sizeof(int64_t));
    if (nkeys) m->keys = nkeys;
    if (!np_ || !nkeys) {
      free(moved);
      free(ki);
      free(first);
      return -1;
    }
    m->cap = cap;
  }
  for (size_t a = 0; a < nf; ++a) memcpy(m->pts + 4 * (m->n + a), moved + 4 * first[a], 4 * sizeof(float));
  /* merge the new points' keys (ki[0 .. nf), ascending) into the sorted key array, from the back */
  {
    size_t w = total, o = m->n;
    for (size_t a = nf; a-- > 0;) {
      while (o > 0 && m->keys[o - 1] > ki[a].key) m->keys[--w] = m->keys[--o];
      m->keys[--w] = ki[a].key;
    }
  }
  m->n = total;
  free(moved);
  free(ki);
  free(first);
  return (long)nf;
}

/* nn cloud of `cloud` seen from `pose`, moved back by pose_inv: out must hold n points; returns the number written */
long orc_map_nn_cloud(const orc_map* m, const float* cloud_xyzw, size_t n, const float pose[16], const float pose_inv[16],
                      float* out_xyzw) {
  if (m->n == 0 || n == 0) return 0;
  int32_t* idx = (int32_t*)malloc(n * sizeof(int32_t));
  float* d2 = (float*)malloc(n * sizeof(float));
  float* sel = (float*)malloc(n * 4 * sizeof(float));
  if (!idx || !d2 || !sel) {
    free(idx);
    free(d2);
    free(sel);
    return -1;
  }
  orc_nn(cloud_xyzw, n, m->pts, m->n, pose, ORC_NN_KDTREE, ORC_ARITH_FMA, idx, d2);
  long k = 0;
  for (size_t i = 0; i < n; ++i)
    if (idx[i] >= 0) memcpy(sel + 4 * (k++), m->pts + 4 * (size_t)idx[i], 4 * sizeof(float));
  orc_transform_cloud(sel, (size_t)k, pose_inv, out_xyzw);
  free(idx);
  free(d2);
  free(sel);
  return k;
}

/* ---- PCL 1.8's OctreePointCloudSearch itself: the tree, addPointsToMap and approxNearestSearch ------------------------
 * A pointer-free restatement of the octree the reference builds (octree_mapper.cpp:55-90): branch nodes with eight child
 * slots, the root re-parented when the box doubles (adoptBoundingBoxToPoint), leaves holding the indices of their points in
 * insertion order (OctreeContainerPointIndices).  Written from PCL's algorithm; nothing here is shared with the lattice form
 * above but the box arithmetic, and nothing with oracle/map_approx_np.py or the kernels. */
struct orc_octree {
  double res;
  orc_box box;
  int32_t root;          /* branch index (-1: no point yet) */
  int32_t (*child)[8];   /* branches; a branch one level above the leaves holds leaf indices */
  size_t nb, cap_b;
  int32_t *head, *tail;  /* leaves: first and last point of each */
  size_t nl, cap_l;
  float* pts;            /* map_cloud_, n x 4 */
  int32_t* next;         /* the next point of the same leaf */
  size_t n, cap;
};

orc_octree* orc_octree_create(double resolution) {
  orc_octree* o = (orc_octree*)calloc(1, sizeof(orc_octree));
  if (o) {
    o->res = resolution;
    o->root = -1;
  }
  return o;
}

void orc_octree_destroy(orc_octree* o) {
  if (!o) return;
  free(o->child);
  free(o->head);
  free(o->tail);
  free(o->pts);
  free(o->next);
  free(o);
}

size_t orc_octree_size(const orc_octree* o) { return o->n; }
const float* orc_octree_points(const orc_octree* o) { return o->pts; }
int orc_octree_depth(const orc_octree* o) { return o->box.defined ? o->box.depth : 0; }
void orc_octree_box(const orc_octree* o, double out[6]) {
  for (int a = 0; a < 3; ++a) {
    out[a] = o->box.min[a];
    out[3 + a] = o->box.max[a];
  }
}

static int32_t octree_new_branch(orc_octree* o) {
  if (o->nb == o->cap_b) {
    const size_t cap = o->cap_b ? 2 * o->cap_b : 1024;
    int32_t(*c)[8] = (int32_t(*)[8])realloc(o->child, cap * sizeof(*c));
    if (!c) return -1;
    o->child = c;
    o->cap_b = cap;
  }
  for (int k = 0; k < 8; ++k) o->child[o->nb][k] = -1;
  return (int32_t)o->nb++;
}

static int32_t octree_new_leaf(orc_octree* o) {
  if (o->nl == o->cap_l) {
    const size_t cap = o->cap_l ? 2 * o->cap_l : 1024;
    int32_t* h = (int32_t*)realloc(o->head, cap * sizeof(int32_t));
    if (h) o->head = h;
    int32_t* t = (int32_t*)realloc(o->tail, cap * sizeof(int32_t));
    if (t) o->tail = t;
    if (!h || !t) return -1;
    o->cap_l = cap;
  }
  o->head[o->nl] = o->tail[o->nl] = -1;
  return (int32_t)o->nl++;
}

static int key_child(const long long k[3], int bit) {
  return (int)((((k[0] >> bit) & 1) << 2) | (((k[1] >> bit) & 1) << 1) | ((k[2] >> bit) & 1));
}

/* existLeaf(genOctreeKeyforPoint(p)) for a point inside the box */
static int octree_leaf_exists(const orc_octree* o, const long long k[3]) {
  int32_t node = o->root;
  for (int d = 1; d <= o->box.depth; ++d) {
    node = o->child[node][key_child(k, o->box.depth - d)];
    if (node < 0) return 0;
  }
  return 1;
}

/* addPointToCloud: adoptBoundingBoxToPoint (a new root per doubling), then createLeafRecursive + addPointIndex */
static int octree_add(orc_octree* o, const float* p) {
  int child;
  while (box_step(&o->box, p, o->res, &child)) {
    const int32_t r = octree_new_branch(o);
    if (r < 0) return -1;
    if (child >= 0) o->child[r][child] = o->root;
    o->root = r;
  }
  long long k[3];
  box_key(&o->box, p, o->res, k);
  int32_t node = o->root;
  for (int d = 1; d <= o->box.depth; ++d) {
    const int c = key_child(k, o->box.depth - d);
    if (o->child[node][c] < 0) {
      const int32_t x = d < o->box.depth ? octree_new_branch(o) : octree_new_leaf(o);
      if (x < 0) return -1;
      o->child[node][c] = x;
    }
    node = o->child[node][c];
  }
  if (o->n == o->cap) {
    const size_t cap = o->cap ? 2 * o->cap : 4096;
    float* np_ = (float*)realloc(o->pts, cap * 4 * sizeof(float));
    if (np_) o->pts = np_;
    int32_t* nx = (int32_t*)realloc(o->next, cap * sizeof(int32_t));
    if (nx) o->next = nx;
    if (!np_ || !nx) return -1;
    o->cap = cap;
  }
  const int32_t i = (int32_t)o->n++;
  memcpy(o->pts + 4 * (size_t)i, p, 3 * sizeof(float));
  o->pts[4 * (size_t)i + 3] = 1.0f;
  o->next[i] = -1;
  if (o->tail[node] >= 0) o->next[o->tail[node]] = i;
  else o->head[node] = i;
  o->tail[node] = i;
  return 0;
}

/* addPointsToMap(transformCloudToPoseFrame(cloud, pose)): "if (!isVoxelOccupiedAtPoint(p)) addPointToCloud(p)" in order.
 * Non-finite points are skipped, and so is a point whose key -- under the box it is tested in, or the box it would grow --
 * lies more than ORC_KEY_REACH voxels from the first box's minimum: the products' reach (21-bit keys), the rule map_candidate
 * states for the lattice form; such a point leaves the box as it was.  PCL itself has no such limit. */
long orc_octree_add_points(orc_octree* o, const float* in_xyzw, size_t n, const float pose[16]) {
  float* moved = (float*)malloc((n ? n : 1) * 4 * sizeof(float));
  if (!moved) return -1;
  if (pose) orc_transform_cloud(in_xyzw, n, pose, moved);
  else memcpy(moved, in_xyzw, n * 4 * sizeof(float));
  long added = 0;
  for (size_t i = 0; i < n; ++i) {
    const float* p = moved + 4 * i;
    orc_box reach = o->box;
    int64_t unused;
    if (!map_candidate(&reach, o->res, p, &unused)) continue; /* non-finite or beyond the reach */
    if (box_inside(&o->box, p)) { /* isVoxelOccupiedAtPoint: false outside the box */
      long long k[3];
      box_key(&o->box, p, o->res, k);
      if (octree_leaf_exists(o, k)) continue;
    }
    if (octree_add(o, p)) {
      free(moved);
      return -1;
    }
    added++;
  }
  free(moved);
  return added;
}

/* pointSquaredDist: (a - b).squaredNorm() in float, (x^2 + y^2) + z^2 */
static float sq_dist(const float* a, const float* b) {
  const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  const float xy = dx * dx + dy * dy;
  return xy + dz * dz;
}

/* approxNearestSearch -> approxNearestSearchRecursive: at every level the existing child whose voxel centre
 * (genVoxelCenterFromOctreeKey, float) is nearest, the first in child order on ties; in the leaf the nearest of its points,
 * the first in insertion order on ties */
static int32_t octree_approx(const orc_octree* o, const float* q) {
  long long key[3] = {0, 0, 0};
  int32_t node = o->root;
  const int depth = o->box.depth;
  for (int d = 1; d <= depth; ++d) {
    const double side = o->res * (double)(1ll << (depth - d));
    double best = DBL_MAX;
    int bc = -1;
    long long bk[3] = {0, 0, 0};
    for (int c = 0; c < 8; ++c) {
      if (o->child[node][c] < 0) continue;
      const long long nk[3] = {2 * key[0] + ((c >> 2) & 1), 2 * key[1] + ((c >> 1) & 1), 2 * key[2] + (c & 1)};
      float ctr[3];
      for (int a = 0; a < 3; ++a) ctr[a] = (float)(((double)nk[a] + 0.5) * side + o->box.min[a]);
      const double dist = (double)sq_dist(ctr, q);
      if (dist >= best) continue;
      best = dist;
      bc = c;
      memcpy(bk, nk, sizeof(bk));
    }
    node = o->child[node][bc];
    memcpy(key, bk, sizeof(key));
  }
  double best = DBL_MAX;
  int32_t r = -1;
  for (int32_t i = o->head[node]; i >= 0; i = o->next[i]) {
    const double dist = (double)sq_dist(o->pts + 4 * (size_t)i, q);
    if (dist >= best) continue;
    best = dist;
    r = i;
  }
  return r;
}

/* idx[i] = approxNearestSearch(pose * cloud[i]); -1 for a non-finite query or an empty map */
void orc_octree_approx_nn(const orc_octree* o, const float* cloud_xyzw, size_t n, const float pose[16], int32_t* idx) {
  for (size_t i = 0; i < n; ++i) {
    float q[4];
    if (pose) orc_transform_cloud(cloud_xyzw + 4 * i, 1, pose, q);
    else memcpy(q, cloud_xyzw + 4 * i, sizeof(q));
    idx[i] = (o->n && isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2])) ? octree_approx(o, q) : -1;
  }
}

/* approxNearestNeighbors(pose * cloud) moved back by pose_inv (the contract of orc_map_nn_cloud); returns the count */
long orc_octree_nn_cloud(const orc_octree* o, const float* cloud_xyzw, size_t n, const float pose[16], const float pose_inv[16],
                         float* out_xyzw) {
  if (o->n == 0 || n == 0) return 0;
  int32_t* idx = (int32_t*)malloc(n * sizeof(int32_t));
  float* sel = (float*)malloc(n * 4 * sizeof(float));
  if (!idx || !sel) {
    free(idx);
    free(sel);
    return -1;
  }
  orc_octree_approx_nn(o, cloud_xyzw, n, pose, idx);
  long k = 0;
  for (size_t i = 0; i < n; ++i)
    if (idx[i] >= 0) memcpy(sel + 4 * (k++), o->pts + 4 * (size_t)idx[i], 4 * sizeof(float));
  orc_transform_cloud(sel, (size_t)k, pose_inv, out_xyzw);
  free(idx);
  free(sel);
  return k;
}
