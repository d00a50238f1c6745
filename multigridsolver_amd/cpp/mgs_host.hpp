// mgs_host.hpp — the C++ face of libmgs.so that keeps the reference's spelling, written on top
// of the C ABI (include/mgs.h) only.  A maintainer of mishraiiit/MultiGridSolver swaps
//     #include "../common/MatrixIO.cpp"   →   #include "mgs_host.hpp" + `using namespace mgs;`
// in src/common/bicg.cpp and keeps `readMatrix`, `SMatrix`, `MultiGridPrecond precond(A, P)`,
// `BiCGSTABiml(A, x, b, precond, max_iter, tol)` as they are.
//
// Reference interfaces mirrored (file:line relative to the reference checkout):
//   SMatrix / readMatrix / writeMatrix        src/common/MatrixIO.cpp:10,12-37,39-57
//   MultiGridPrecond(A,P), solve(v)           src/common/bicg.cpp:19-62
//   dot / norm / BiCGSTABiml                  src/common/bicg.cpp:64-136
//   CGiml (pcg of the Matlab driver)          src/CPU_Matlab/solve.m:28-31
//   TicToc / printScreen                      src/CPU_C++/TicToc.cpp:18-53
#pragma once
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mgs.h"

namespace mgs {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string &m) : std::runtime_error("libmgs error " + std::to_string(c) + ": " + m), code(c) {}
};
inline void check(int rc, const mgs_ctx *ctx = nullptr) {
  if (rc != MGS_OK) { const char *m = mgs_last_error(ctx); throw Error(rc, m ? m : "?"); }
}

// one process-wide context (the reference is single-device, single-thread: SURVEY §0 G5)
inline mgs_ctx *context() {
  static mgs_ctx *ctx = [] {
    mgs_ctx *c = nullptr;
    const char *dev = std::getenv("MGS_DEVICE");
    check(mgs_ctx_create(dev ? std::atoi(dev) : 0, nullptr, &c));
    return c;
  }();
  return ctx;
}

// ---------------------------------------------------------------- host CSR: `SMatrix`
// Eigen::SparseMatrix<double,RowMajor> stand-in (MatrixIO.cpp:10): f64 values, int32 indices,
// sorted columns.  Only the members the reference's drivers use are provided.
struct SMatrix {
  int m_rows = 0, m_cols = 0;
  std::vector<int> rowptr{0}, col;
  std::vector<double> val;
  int rows() const { return m_rows; }
  int cols() const { return m_cols; }
  int nonZeros() const { return (int)col.size(); }
};

inline SMatrix readMatrix(std::string filename) {          // MatrixIO.cpp:12-37
  SMatrix A; int nnz = 0; int *rp = nullptr, *ci = nullptr; double *v = nullptr;
  check(mgs_mtx_read(filename.c_str(), &A.m_rows, &A.m_cols, &nnz, &rp, &ci, &v));
  A.rowptr.assign(rp, rp + A.m_rows + 1); A.col.assign(ci, ci + nnz); A.val.assign(v, v + nnz);
  mgs_host_free(rp); mgs_host_free(ci); mgs_host_free(v);
  return A;
}
inline void writeMatrix(std::string filename, const SMatrix &A) {   // MatrixIO.cpp:39-57
  check(mgs_mtx_write(filename.c_str(), A.rows(), A.cols(), A.nonZeros(), A.rowptr.data(), A.col.data(), A.val.data()));
}

// ---------------------------------------------------------------- device vector: `VectorXd`
// Value semantics like Eigen::VectorXd (copies are deep); arithmetic runs on the device.
class Vector {
  std::shared_ptr<mgs_vec> v_;
  // Host staging for element access (`b[i] = …`, `x(0)`: bicg.cpp:78,159-162).  The first access downloads the vector once;
  // writes mark the mirror dirty and the next device use (handle()) uploads it.  Plain device arithmetic never touches it.
  mutable std::vector<double> host_;
  mutable bool host_valid_ = false, host_dirty_ = false;
  static std::shared_ptr<mgs_vec> make(int64_t n) {
    mgs_vec *p = nullptr; check(mgs_vec_create(context(), n, &p), context());
    return std::shared_ptr<mgs_vec>(p, [](mgs_vec *q) { mgs_vec_destroy(q); });
  }
  void flush() const {
    if (host_dirty_) { check(mgs_vec_upload(v_.get(), host_.data(), (int64_t)host_.size()), context()); host_dirty_ = false; }
  }
  double *stage() const {
    if (!host_valid_) { host_.resize((size_t)size()); if (size()) check(mgs_vec_download(v_.get(), host_.data(), size()), context()); host_valid_ = true; }
    return host_.data();
  }
 public:
  Vector() {}
  explicit Vector(int64_t n) : v_(make(n)) {}
  Vector(const Vector &o) { if (o.v_) { v_ = make(o.size()); check(mgs_vec_copy(o.handle(), v_.get()), context()); } }
  Vector(Vector &&) = default;
  Vector &operator=(const Vector &o) { if (this != &o) { Vector t(o); v_ = std::move(t.v_); host_valid_ = host_dirty_ = false; } return *this; }
  Vector &operator=(Vector &&) = default;
  int64_t size() const { return v_ ? mgs_vec_size(v_.get()) : 0; }
  int64_t rows() const { return size(); }
  // device handle for reading: pending element writes are uploaded first
  mgs_vec *handle() const { flush(); return v_.get(); }
  // device handle for writing: the host mirror no longer reflects the device
  mgs_vec *out() { flush(); host_valid_ = false; return v_.get(); }
  double &operator[](int64_t i) { double *h = stage(); host_dirty_ = true; return h[i]; }          // bicg.cpp:161
  double operator[](int64_t i) const { return stage()[i]; }
  double &operator()(int64_t i) { return (*this)[i]; }                                              // bicg.cpp:78 style access
  double operator()(int64_t i) const { return (*this)[i]; }
  void setZero() { check(mgs_vec_fill(out(), 0.0), context()); }
  void upload(const std::vector<double> &h) { check(mgs_vec_upload(out(), h.data(), (int64_t)h.size()), context()); }
  std::vector<double> download() const { std::vector<double> h((size_t)size()); check(mgs_vec_download(handle(), h.data(), size()), context()); return h; }
  // y[k] = (*this)[idx[k]] and x[idx[k]] = (*this)[k] for k < n (mgs.h: mgs_vec_gather, mgs_vec_scatter, in the C argument order): idx in
  // device memory, index_bits 32 or 64; an index outside the indexed vector is never used (gather stores +0.0, scatter skips it).
  // Without `bad` the call is enqueued only; with it the call synchronises, writes the number of such indices and throws
  // Error(MGS_ERR_INVALID) when that is not 0.
  void gather(const void *idx_dev, int64_t n, int index_bits, Vector &y, int64_t *bad = nullptr) const {
    check(mgs_vec_gather(handle(), idx_dev, n, index_bits, y.out(), bad), context());
  }
  void scatter(const void *idx_dev, int64_t n, int index_bits, Vector &x, int64_t *bad = nullptr) const {
    check(mgs_vec_scatter(handle(), idx_dev, n, index_bits, x.out(), bad), context());
  }
  double dot(const Vector &o) const { double s; check(mgs_dot(handle(), o.handle(), &s), context()); return s; }
  double norm() const { double s; check(mgs_nrm2(handle(), &s), context()); return s; }
  Vector &operator+=(const Vector &o) { check(mgs_axpby(1.0, o.handle(), 1.0, out()), context()); return *this; }
  Vector &operator-=(const Vector &o) { check(mgs_axpby(-1.0, o.handle(), 1.0, out()), context()); return *this; }
  friend Vector operator+(const Vector &a, const Vector &b) { Vector r(a.size()); check(mgs_axpbypcz(1.0, a.handle(), 1.0, b.handle(), 0.0, r.out()), context()); return r; }
  friend Vector operator-(const Vector &a, const Vector &b) { Vector r(a.size()); check(mgs_axpbypcz(1.0, a.handle(), -1.0, b.handle(), 0.0, r.out()), context()); return r; }
  friend Vector operator*(double s, const Vector &a) { Vector r(a.size()); check(mgs_axpby(s, a.handle(), 0.0, r.out()), context()); return r; }
  friend Vector operator*(const Vector &a, double s) { return s * a; }
};
typedef Vector VectorXd;

// ---------------------------------------------------------------- device operator: `A * v`
class DeviceMatrix {
  std::shared_ptr<mgs_csr> a_;
  int rows_ = 0, cols_ = 0;
  static DeviceMatrix adopt(mgs_csr *p, int rows, int cols) {
    DeviceMatrix M; M.rows_ = rows; M.cols_ = cols;
    M.a_ = std::shared_ptr<mgs_csr>(p, [](mgs_csr *q) { mgs_csr_destroy(q); });
    return M;
  }
  static std::vector<const mgs_csr *> handles(int br, int bc, const DeviceMatrix *const *blocks) {   // a grid of blocks as the C-ABI takes it
    std::vector<const mgs_csr *> h((size_t)(br > 0 ? br : 0) * (size_t)(bc > 0 ? bc : 0), nullptr);
    for (size_t q = 0; q < h.size(); ++q) h[q] = blocks && blocks[q] ? blocks[q]->a_.get() : nullptr;
    return h;
  }
 public:
  DeviceMatrix() {}
  DeviceMatrix(const SMatrix &A) : rows_(A.rows()), cols_(A.cols()) {
    mgs_csr *p = nullptr;
    check(mgs_csr_upload(context(), A.rows(), A.cols(), A.nonZeros(), A.rowptr.data(), A.col.data(), A.val.data(), &p), context());
    a_ = std::shared_ptr<mgs_csr>(p, [](mgs_csr *q) { mgs_csr_destroy(q); });
  }
  // Arrays that already live in device memory (mgs.h: mgs_csr_from_device / mgs_csr_from_coo_device; index_bits 32 or 64).  The
  // inputs are checked on the device and copied; bad input throws Error(MGS_ERR_INVALID).  Triples may come in any order and
  // duplicates are summed in input order; keep_map keeps what update_values_coo needs.
  static DeviceMatrix fromDevice(int rows, int cols, int64_t nnz, const void *rowptr, const void *col, int index_bits, const void *val) {
    mgs_csr *p = nullptr;
    check(mgs_csr_from_device(context(), rows, cols, nnz, rowptr, col, index_bits, val, &p), context());
    return adopt(p, rows, cols);
  }
  static DeviceMatrix fromCooDevice(int rows, int cols, int64_t ntrip, const void *row, const void *col, int index_bits, const void *val, bool keep_map = false) {
    mgs_csr *p = nullptr;
    check(mgs_csr_from_coo_device(context(), rows, cols, ntrip, row, col, index_bits, val, keep_map ? 1 : 0, &p), context());
    return adopt(p, rows, cols);
  }
  // new triple values (device memory, same triples in the same order) through the kept map; enqueued, not synchronised
  void update_values_coo(const void *val_dev, int64_t ntrip) { check(mgs_csr_update_values_coo_dev(a_.get(), val_dev, ntrip), context()); }
  int rows() const { return rows_; }
  int cols() const { return cols_; }
  mgs_csr *handle() const { return a_.get(); }
  // Declares A·1 = 0 and 1ᵀ·A = 0 (pure-Neumann operators, graph Laplacians; mgs.h: mgs_csr_set_nullspace) — or takes the declaration
  // back.  Set it before MultiGridPrecond is built on this matrix: its coarsest solve is then regularised, and BiCGSTABiml / CGiml
  // solve A·x = Πb and return the x of zero mean.  Copies of a DeviceMatrix share the device matrix and with it the declaration.
  void setNullspaceConstant(bool on) { check(mgs_csr_set_nullspace(a_.get(), on ? MGS_NULLSPACE_CONSTANT : MGS_NULLSPACE_NONE), context()); }
  bool nullspaceConstant() const { int k = 0; check(mgs_csr_nullspace(a_.get(), &k), context()); return k == MGS_NULLSPACE_CONSTANT; }
  // Declares a field-wise constant null space (mgs.h: mgs_csr_set_nullspace_fields): labels_dev holds rows() entries of index_bits (32 or
  // 64) bits in DEVICE memory, f in [0, nfields) puts the row in field f, −1 in no field — the pressure constant of enclosed Stokes flow,
  // one constant per component of a graph Laplacian.  Checked on the device and copied; served by MINRESiml / MinresPlan and CGiml.
  // setNullspaceConstant(false) takes the declaration back.  nullspaceFields(): the rows of every declared field (empty: another kind).
  void setNullspaceFields(const void *labels_dev, int index_bits, int nfields) { check(mgs_csr_set_nullspace_fields(a_.get(), labels_dev, index_bits, nfields), context()); }
  std::vector<int64_t> nullspaceFields() const {
    int nf = 0; int64_t cnt[MGS_NULLSPACE_MAX_FIELDS];
    check(mgs_csr_nullspace_fields(a_.get(), &nf, cnt), context());
    return std::vector<int64_t>(cnt, cnt + nf);
  }
  // New values, same pattern, in place (mgs.h: mgs_csr_update_values; the reference would upload a new matrix).  The pattern of A is
  // compared with the device copy's on the host: a different rowptr / col throws Error(MGS_ERR_INVALID).
  void update_values(const SMatrix &A) {
    int r = 0, c = 0; int64_t nnz = 0;
    check(mgs_csr_shape(a_.get(), &r, &c, &nnz), context());
    bool same = r == A.rows() && c == A.cols() && nnz == (int64_t)A.nonZeros() && (int)A.rowptr.size() == r + 1;
    if (same) {
      std::vector<int> rp((size_t)r + 1), ci((size_t)nnz + 1);
      check(mgs_csr_download(a_.get(), rp.data(), ci.data(), nullptr), context());
      ci.resize((size_t)nnz);
      same = rp == A.rowptr && ci == A.col;
    }
    if (!same) throw Error(MGS_ERR_INVALID, "DeviceMatrix::update_values: the sparsity pattern differs from the uploaded matrix's");
    check(mgs_csr_update_values(a_.get(), A.val.data(), nnz), context());
  }
  // C = (*this)·B on the device (mgs.h: mgs_csr_spgemm; the Eigen products of bicg.cpp:32-33): structural pattern, ascending columns,
  // products summed in storage order.  multiplyUpdate: this matrix is A.multiply(B) built earlier — its values again, in place, from
  // the current values of A and B with their patterns unchanged (mgs_csr_spgemm_numeric).  Without `misses` the call is enqueued
  // only; with it the call synchronises, writes the number of products outside this matrix's pattern and throws Error(MGS_ERR_STATE)
  // when that is not 0.
  DeviceMatrix multiply(const DeviceMatrix &B) const {
    mgs_csr *p = nullptr;
    check(mgs_csr_spgemm(a_.get(), B.a_.get(), &p), context());
    return adopt(p, rows_, B.cols_);
  }
  void multiplyUpdate(const DeviceMatrix &A, const DeviceMatrix &B, int64_t *misses = nullptr) {
    check(mgs_csr_spgemm_numeric(A.a_.get(), B.a_.get(), a_.get(), misses), context());
  }
  // C = alpha·(*this) + beta·B on the device (mgs.h: mgs_csr_add; no reference counterpart): the union of the two patterns, ascending
  // columns, every product and sum rounded on its own.  addUpdate: this matrix is A.add(B, ...) built earlier — its values again, in
  // place, from the current values of A and B with their patterns unchanged and the scalars given here (mgs_csr_add_numeric); `misses`
  // as in multiplyUpdate.  scale: a_ij ← (dl_i·a_ij)·dr_j in place, either vector may be NULL (mgs_csr_scale; enqueued).  diagonal /
  // fromDiagonal: the diagonal as a vector (0 where none is stored) and a vector as a diagonal matrix (mgs_csr_diag, mgs_csr_from_diag).
  DeviceMatrix add(const DeviceMatrix &B, double alpha = 1.0, double beta = 1.0) const {
    mgs_csr *p = nullptr;
    check(mgs_csr_add(alpha, a_.get(), beta, B.a_.get(), &p), context());
    return adopt(p, rows_, cols_);
  }
  void addUpdate(const DeviceMatrix &A, const DeviceMatrix &B, double alpha = 1.0, double beta = 1.0, int64_t *misses = nullptr) {
    check(mgs_csr_add_numeric(alpha, A.a_.get(), beta, B.a_.get(), a_.get(), misses), context());
  }
  void scale(const Vector *dl, const Vector *dr) {
    check(mgs_csr_scale(a_.get(), dl ? dl->handle() : nullptr, dr ? dr->handle() : nullptr), context());
  }
  Vector diagonal() const {
    Vector d(rows_ < cols_ ? rows_ : cols_); check(mgs_csr_diag(a_.get(), d.out()), context()); return d;
  }
  static DeviceMatrix fromDiagonal(const Vector &d) {
    mgs_csr *p = nullptr;
    check(mgs_csr_from_diag(context(), d.handle(), &p), context());
    return adopt(p, (int)d.size(), (int)d.size());
  }
  // S = (*this)(rows, cols) on the device (mgs.h: mgs_csr_extract; no reference counterpart): index lists in device memory, index_bits 32
  // or 64 for both; a NULL list means every row / every column (its length is then ignored).  Rows in any order, repeats allowed;
  // columns strictly ascending, column cols[q] becomes q; value bits are copied unchanged.  keepMap keeps what extractUpdate needs.
  // extractUpdate: this matrix is A.extract(..., keepMap = true) built earlier — its values again, in place, from the current values
  // of A with its pattern unchanged (mgs_csr_extract_numeric; enqueued, no host wait).
  DeviceMatrix extract(const void *rows_dev, int64_t nr, const void *cols_dev, int64_t nc, int index_bits = 32, bool keepMap = false) const {
    mgs_csr *p = nullptr;
    check(mgs_csr_extract(a_.get(), rows_dev, nr, cols_dev, nc, index_bits, keepMap ? 1 : 0, &p), context());
    return adopt(p, rows_dev ? (int)nr : rows_, cols_dev ? (int)nc : cols_);
  }
  void extractUpdate(const DeviceMatrix &A) { check(mgs_csr_extract_numeric(A.a_.get(), a_.get()), context()); }
  // C = (*this)(rperm, cperm) for two permutations in device memory (mgs.h: mgs_csr_permute; no reference counterpart): C(i, j) =
  // (*this)(rperm[i], cperm[j]); rows() and cols() entries of index_bits 32 or 64 for both; a NULL list is the identity.  Each list must
  // be a bijection (checked on the device); a symmetric reordering passes the same list twice.  keepMap keeps what permuteUpdate needs.
  // permuteUpdate: this matrix is A.permute(..., keepMap = true) built earlier — its values again, in place, from the current values of
  // A with its pattern unchanged (mgs_csr_permute_numeric; enqueued, no host wait).
  DeviceMatrix permute(const void *rperm_dev, const void *cperm_dev, int index_bits = 32, bool keepMap = false) const {
    mgs_csr *p = nullptr;
    check(mgs_csr_permute(a_.get(), rperm_dev, cperm_dev, index_bits, keepMap ? 1 : 0, &p), context());
    return adopt(p, rows_, cols_);
  }
  void permuteUpdate(const DeviceMatrix &A) { check(mgs_csr_permute_numeric(A.a_.get(), a_.get()), context()); }
  // The matrix assembled from a br × bc grid of blocks, row-major (mgs.h: mgs_csr_bmat; scipy.sparse.bmat): a NULL pointer is a zero
  // block, the same matrix may appear in several places; row_sizes / col_sizes (br / bc ints, or NULL) are needed only where a whole
  // block row or column is NULL.  bmatUpdate: this matrix is bmat(...) built earlier — its values again, in place, from the current
  // values of the blocks with their patterns unchanged (mgs_csr_bmat_numeric; one launch).
  static DeviceMatrix bmat(int br, int bc, const DeviceMatrix *const *blocks, const int *row_sizes = nullptr, const int *col_sizes = nullptr) {
    std::vector<const mgs_csr *> h = handles(br, bc, blocks);
    mgs_csr *p = nullptr;
    check(mgs_csr_bmat(context(), br, bc, h.data(), row_sizes, col_sizes, &p), context());
    int r = 0, c = 0;
    check(mgs_csr_shape(p, &r, &c, nullptr), context());
    return adopt(p, r, c);
  }
  void bmatUpdate(int br, int bc, const DeviceMatrix *const *blocks) {
    int64_t info[4] = {0, 0, 0, 0};      // the C call takes no grid dimensions: it reads as many handles as this matrix recorded
    check(mgs_csr_bmat_info(a_.get(), info), context());
    if (info[1] != br || info[2] != bc)
      throw Error(MGS_ERR_INVALID, "DeviceMatrix::bmatUpdate: a grid of " + std::to_string(br) + " x " + std::to_string(bc) + " blocks given, this matrix was assembled from " +
                                       std::to_string((long long)info[1]) + " x " + std::to_string((long long)info[2]));
    std::vector<const mgs_csr *> h = handles(br, bc, blocks);
    check(mgs_csr_bmat_numeric(a_.get(), h.data()), context());
  }
  // The transpose, materialised row-major (mgs.h: mgs_csr_transpose; bicg.cpp:32).  transposeUpdate: this matrix is A.transpose() built
  // earlier — its values again, in place, from the current values of A with its pattern unchanged (mgs_csr_transpose_numeric; one
  // launch, no kept map).  Without `misses` the call is enqueued only; with it the call synchronises, writes the number of entries of A
  // without a place here and throws Error(MGS_ERR_STATE) when that is not 0.  A scale() applied to this matrix is applied again afterwards.
  DeviceMatrix transpose() const {
    mgs_csr *p = nullptr;
    check(mgs_csr_transpose(a_.get(), &p), context());
    return adopt(p, cols_, rows_);
  }
  void transposeUpdate(const DeviceMatrix &A, int64_t *misses = nullptr) { check(mgs_csr_transpose_numeric(A.a_.get(), a_.get(), misses), context()); }
  Vector operator*(const Vector &x) const {            // bicg.cpp:57,82,107,117
    Vector y(rows_); check(mgs_spmv(a_.get(), x.handle(), y.out()), context()); return y;
  }
};

// ---------------------------------------------------------------- MultiGridPrecond (bicg.cpp:19-62)
// Same constructor and solve() shape.  The coarse direct solve + ILUT smoother of the reference
// are replaced by the V-cycle of this library: P gives level 1, further levels are aggregated on
// the device until the coarsest has ≤ coarse_rows rows (then inverted densely on the device);
// smoother = damped Jacobi (solve.m:17).  With levels == 2, nu1 == 0, nu2 == 1 solve() is exactly
// bicg.cpp:46-61 with M2 = ωD⁻¹.
struct PrecondOptions {
  double omega = 0.6; int nu1 = 1, nu2 = 1;
  double correction_scale = 1.0;                         // x ← x + σ·P e_c; 1 = the reference's form (bicg.cpp:48)
  double ktg = 10.0; int npass = 2; double tou = 8.0;   // src/GPU_CUDAC++/results.txt:22-24
  int coarse_rows = 2500; int max_levels = 32;   // ≤ 2500 rows: dense inverse (a GEMV beats two more latency-bound levels)
  // the two switches of the reference's solve() (bicg.cpp:42-43,53-59; both fixed to true there):
  bool multiplicative_precond = true;   // false: multigrid_solve(v) + M2(v) (:59) with M2 = ωD⁻¹
  bool use_preconditioner = true;       // false: solve(v) = v (:53-54)
};
class MultiGridPrecond {
  DeviceMatrix A_;
  std::shared_ptr<mgs_hier> h_;
  bool use_preconditioner_ = true, symmetric_ = true;
 public:
  typedef PrecondOptions Options;
  MultiGridPrecond(const SMatrix &A_in, const SMatrix &P_in, Options o = Options()) : A_(A_in) { build(A_, &P_in, o); }
  MultiGridPrecond(const DeviceMatrix &A_dev, const SMatrix *P_in, Options o = Options()) : A_(A_dev) { build(A_, P_in, o); }
  template <typename T> T solve(const T &vec) const {     // bicg.cpp:51-61
    if (!use_preconditioner_) return vec;                  // :53-54
    T out(vec.size());
    check(mgs_vcycle(h_.get(), vec.handle(), out.out(), 1), context());
    return out;
  }
  bool use_preconditioner() const { return use_preconditioner_; }
  bool symmetric() const { return symmetric_; }          // nu1 == nu2: the cycle is a fixed symmetric operator (CGiml's classical β applies)
  mgs_hier *handle() const { return h_.get(); }
  const DeviceMatrix &matrix() const { return A_; }
  int levels() const { return mgs_hier_nlev(h_.get()); }
  // stored precision of the cycle's matrix operands (mgs.h: mgs_hier_set_operand_precision; the reference's GPU path keeps its matrices in
  // float32, src/GPU_CUDAC++/MatrixIO.cu:32-36): bits = 64 | 32, on at most `levels` leading levels (< 0: every eligible one)
  void set_operand_precision(int bits, int levels = -1) { check(mgs_hier_set_operand_precision(h_.get(), bits, levels), context()); }
  int operand_precision(int level) const { int bits = 64; check(mgs_hier_operand_precision(h_.get(), level, &bits), context()); return bits; }
  // Values changed, pattern did not (mgs.h: mgs_hier_refresh; the reference reruns its constructor per matrix, bicg.cpp:19-44): the
  // aggregates and everything that depends on the pattern only are kept, the numbers are recomputed on the device.  refresh() reads
  // the device matrix as it stands (after DeviceMatrix::update_values on the matrix handed to the constructor); refresh(A_new)
  // first writes A_new's values into the preconditioner's matrix — its own upload for the (SMatrix, SMatrix) constructor, the
  // caller's shared one otherwise — and throws Error(MGS_ERR_INVALID) if A_new's pattern differs.
  void refresh() { check(mgs_hier_refresh(h_.get()), context()); }
  void refresh(const SMatrix &A_new) { A_.update_values(A_new); refresh(); }
 private:
  void build(const DeviceMatrix &A, const SMatrix *P, const Options &o) {
    mgs_hier *h = nullptr;
    check(mgs_hier_create(context(), A.handle(), o.omega, o.nu1, o.nu2, &h), context());
    h_ = std::shared_ptr<mgs_hier>(h, [](mgs_hier *q) { mgs_hier_destroy(q); });
    if (P) { DeviceMatrix Pd(*P); check(mgs_hier_push_P(h, Pd.handle()), context()); }
    check(mgs_hier_coarsen(h, o.ktg, o.npass, o.tou, o.coarse_rows, o.max_levels), context());
    check(mgs_hier_finalize(h), context());
    if (!o.multiplicative_precond) check(mgs_hier_set_additive(h, 1), context());
    if (o.correction_scale != 1.0) check(mgs_hier_set_correction_scale(h, o.correction_scale), context());
    use_preconditioner_ = o.use_preconditioner; symmetric_ = o.nu1 == o.nu2;
  }
};

// ---------------------------------------------------------------- bicg.cpp:64-72
template <typename V> inline double dot(const V &A, const V &B) { return A.dot(B); }
template <typename V> inline double norm(const V &A) { return A.norm(); }

// BiCGSTABiml, bicg.cpp:74-136: same signature, status codes (0 ok / 1 max_iter / 2 rho = 0 /
// 3 omega = 0) and write-back of max_iter / tol.  Generic form: works with any Matrix providing
// operator*(Vector) and any Preconditioner providing solve(Vector); scalars are plain Reals (the
// reference keeps them in 1-element Vectors, :78).
template <class Matrix, class Vec, class Preconditioner, class Real>
int BiCGSTABiml(const Matrix &A, Vec &x, const Vec &b, const Preconditioner &M, int &max_iter, Real &tol) {
  Real resid, rho_1 = 0, rho_2 = 0, alpha = 0, beta = 0, omega = 0;
  Vec p, phat, s, shat, t, v;
  Real normb = norm(b);
  Vec r = b - A * x;
  Vec rtilde = r;
  if (normb == 0.0) normb = 1;
  if ((resid = norm(r) / normb) <= tol) { tol = resid; max_iter = 0; return 0; }
  for (int i = 1; i <= max_iter; i++) {
    rho_1 = dot(rtilde, r);
    if (rho_1 == 0) { tol = norm(r) / normb; return 2; }
    if (i == 1) p = r;
    else { beta = (rho_1 / rho_2) * (alpha / omega); p = r + beta * (p - omega * v); }
    phat = M.solve(p);
    v = A * phat;
    alpha = rho_1 / dot(rtilde, v);
    s = r - alpha * v;
    if ((resid = norm(s) / normb) < tol) { x += alpha * phat; max_iter = i; tol = resid; return 0; }
    shat = M.solve(s);
    t = A * shat;
    omega = dot(t, s) / dot(t, t);
    x += alpha * phat + omega * shat;
    r = s - omega * t;
    rho_2 = rho_1;
    if ((resid = norm(r) / normb) < tol) { tol = resid; max_iter = i; return 0; }
    if (omega == 0) { tol = norm(r) / normb; return 3; }
  }
  tol = resid;
  return 1;
}
// Device-resident fast path for the library's own types (no temporaries, fused updates):
inline int BiCGSTABiml(const DeviceMatrix &A, Vector &x, const Vector &b, const MultiGridPrecond &M, int &max_iter, double &tol) {
  int status = -1;
  check(mgs_bicgstab(A.handle(), x.out(), b.handle(), M.use_preconditioner() ? M.handle() : nullptr, &max_iter, &tol, &status), context());
  return status;
}
// the call exactly as the reference's main() writes it (bicg.cpp:168): A is the host SMatrix the preconditioner was built
// from — its device copy lives in M
inline int BiCGSTABiml(const SMatrix &, Vector &x, const Vector &b, const MultiGridPrecond &M, int &max_iter, double &tol) {
  return BiCGSTABiml(M.matrix(), x, b, M, max_iter, tol);
}

// Preconditioned CG for symmetric positive definite A (the reference's Matlab driver, src/CPU_Matlab/solve.m:28-31), in the calling
// shape of BiCGSTABiml.  Status: 0 ok (confirmed on the true residual b − A·x) / 1 max_iter / 2 r·z not positive / 3 p·A·p not
// positive; max_iter and tol are written back.  Generic form (classical β = ρ/ρ_prev): any Matrix with operator*(Vec), any
// Preconditioner with solve(Vec) that is a fixed symmetric positive operator.
template <class Matrix, class Vec, class Preconditioner, class Real>
int CGiml(const Matrix &A, Vec &x, const Vec &b, const Preconditioner &M, int &max_iter, Real &tol) {
  Real resid, rho = 0, rho_prev = 0, alpha = 0, pq = 0;
  Vec p, z, q;
  Real normb = norm(b);
  Vec r = b - A * x;
  if (normb == 0.0) normb = 1;
  if ((resid = norm(r) / normb) <= tol) { tol = resid; max_iter = 0; return 0; }
  bool restart = true;
  for (int i = 1; i <= max_iter; i++) {
    z = M.solve(r);
    rho = dot(r, z);
    if (!(rho > 0)) { tol = resid; max_iter = i; return 2; }
    if (restart) { p = z; restart = false; }
    else p = z + (rho / rho_prev) * p;
    q = A * p;
    pq = dot(p, q);
    if (!(pq > 0)) { tol = resid; max_iter = i; return 3; }
    alpha = rho / pq;
    x += alpha * p;
    r -= alpha * q;
    resid = norm(r) / normb;
    rho_prev = rho;
    if (resid < tol) {
      r = b - A * x;
      if ((resid = norm(r) / normb) < tol) { tol = resid; max_iter = i; return 0; }
      restart = true;
    }
  }
  tol = resid;
  return 1;
}
// Device-resident fast path (mgs_pcg: four work vectors, three fused vector passes per iteration beside cycle and SpMV).  The
// flexible β is chosen where the hierarchy is not a fixed symmetric operator (nu1 != nu2): mgs_pcg refuses the classical form there.
inline int CGiml(const DeviceMatrix &A, Vector &x, const Vector &b, const MultiGridPrecond &M, int &max_iter, double &tol) {
  int status = -1;
  check(mgs_pcg(A.handle(), x.out(), b.handle(), M.use_preconditioner() ? M.handle() : nullptr, M.symmetric() ? 0 : 1, &max_iter, &tol, &status), context());
  return status;
}
// with the host SMatrix the preconditioner was built from, as the reference's main() calls its solver (bicg.cpp:168)
inline int CGiml(const SMatrix &, Vector &x, const Vector &b, const MultiGridPrecond &M, int &max_iter, double &tol) {
  return CGiml(M.matrix(), x, b, M, max_iter, tol);
}

// Preconditioned MINRES for symmetric A that may be indefinite (saddle-point systems), in the calling shape of BiCGSTABiml.  The reference
// has no MINRES: its Matlab driver, src/CPU_Matlab/solve.m:28-33, chooses between pcg and bicgstab.  Status: 0 ok (confirmed on the true
// residual b − A·x) / 1 max_iter / 2 z̃·v negative or not a number (M is not positive definite) / 3 Krylov space exhausted above the
// tolerance; max_iter is written back, and tol with the TRUE relative residual whatever the status.  Generic form (mgs.h: mgs_minres states
// the recurrence): any Matrix with operator*(Vec), any Preconditioner with solve(Vec) that is a fixed symmetric positive definite operator.
template <class Matrix, class Vec, class Preconditioner, class Real>
int MINRESiml(const Matrix &A, Vec &x, const Vec &b, const Preconditioner &M, int &max_iter, Real &tol) {
  Real normb = norm(b);
  if (normb == 0.0) normb = 1;
  Vec v = b - A * x, v_prev = 0.0 * v, w = v_prev, w_prev = v_prev, q;
  Real resid = norm(v) / normb;
  if (resid <= tol) { tol = resid; max_iter = 0; return 0; }
  Vec z = M.solve(v);
  Real g2 = dot(z, v);
  if (!(g2 > 0)) { tol = resid; max_iter = 0; return 2; }
  Real gam = std::sqrt(g2), gam_prev = 1, eta = gam, kappa = resid * normb / gam, s0 = 0, s1 = 0, c0 = 1, c1 = 1;
  auto true_resid = [&]() { q = b - A * x; return Real(norm(q) / normb); };
  const int maxit = max_iter;
  for (int j = 1; j <= maxit; j++) {
    q = A * z;
    const Real delta = dot(q, z) / (gam * gam);
    Vec v_new = (1.0 / gam) * q - (delta / gam) * v - (gam / gam_prev) * v_prev;
    Vec z_new = M.solve(v_new);
    const Real gn2 = dot(z_new, v_new);
    if (!(gn2 >= 0)) { tol = true_resid(); max_iter = j; return 2; }
    const Real gamn = std::sqrt(gn2);
    const Real a0 = c1 * delta - c0 * s1 * gam, a1 = std::sqrt(a0 * a0 + gn2), a2 = s1 * delta + c0 * c1 * gam, a3 = s0 * gam;
    if (a1 == 0) { tol = true_resid(); max_iter = j; return 3; }
    const Real cn = a0 / a1, sn = gamn / a1;
    Vec w_new = (1.0 / a1) * ((1.0 / gam) * z - a3 * w_prev - a2 * w);      // (Vec need not offer a quotient; the device path divides)
    x += (cn * eta) * w_new;
    eta = -sn * eta;
    v_prev = v; v = v_new; z = z_new; w_prev = w; w = w_new;
    s0 = s1; s1 = sn; c0 = c1; c1 = cn; gam_prev = gam; gam = gamn;
    bool fresh = false;
    if (kappa * std::fabs(eta) / normb < tol || gamn == 0) {
      resid = true_resid(); fresh = true;
      if (resid < tol) { tol = resid; max_iter = j; return 0; }
      if (gamn == 0) { tol = resid; max_iter = j; return 3; }
      kappa = resid * normb / std::fabs(eta);
    }
    if (j == maxit && !fresh) resid = true_resid();
  }
  tol = resid;
  return 1;
}
// Device-resident fast path (mgs_minres: seven work vectors, one cycle and one SpMV per iteration).  The hierarchy must be a fixed symmetric
// operator (nu1 == nu2, no K-cycle): mgs_minres refuses any other, and there is no flexible form to fall back to.
inline int MINRESiml(const DeviceMatrix &A, Vector &x, const Vector &b, const MultiGridPrecond &M, int &max_iter, double &tol) {
  int status = -1;
  check(mgs_minres(A.handle(), x.out(), b.handle(), M.use_preconditioner() ? M.handle() : nullptr, &max_iter, &tol, &status), context());
  return status;
}
// with the host SMatrix the preconditioner was built from, as the reference's main() calls its solver (bicg.cpp:168)
inline int MINRESiml(const SMatrix &, Vector &x, const Vector &b, const MultiGridPrecond &M, int &max_iter, double &tol) {
  return MINRESiml(M.matrix(), x, b, M, max_iter, tol);
}

// ---------------------------------------------------------------- block vectors and the smallest eigenpairs (mgs.h: mgs_vecs_*, mgs_eig_lobpcg)
// No reference counterpart: the reference solves linear systems, one vector at a time.  A block is a std::vector<Vector>.
// G = UᵀV, row-major U.size() × V.size(), bit-reproducible; the same block on both sides gives a G that is symmetric bit for bit
inline std::vector<double> vecsGram(const std::vector<Vector> &U, const std::vector<Vector> &V) {
  std::vector<const mgs_vec *> u, v;
  for (const Vector &c : U) u.push_back(c.handle());
  for (const Vector &c : V) v.push_back(c.handle());
  std::vector<double> G(U.size() * V.size());
  check(mgs_vecs_gram(context(), U.empty() ? 0 : U[0].size(), (int)u.size(), u.data(), (int)v.size(), v.data(), G.data()), context());
  return G;
}
// Y_j = Σ_a C[a·Y.size() + j]·S_a, added in ascending a; Y may be S itself (or share whole columns with it)
inline void vecsCombine(const std::vector<Vector> &S, const std::vector<double> &C, std::vector<Vector> &Y) {
  if (C.size() != S.size() * Y.size()) throw Error(MGS_ERR_INVALID, "vecsCombine: C is not S.size() x Y.size()");
  std::vector<const mgs_vec *> s;
  std::vector<mgs_vec *> y;
  for (const Vector &c : S) s.push_back(c.handle());
  for (Vector &c : Y) y.push_back(c.out());
  check(mgs_vecs_combine(context(), S.empty() ? 0 : S[0].size(), (int)s.size(), s.data(), (int)y.size(), y.data(), C.data()), context());
}
// The X.size() smallest eigenpairs of the symmetric A (mgs_eig_lobpcg), in the calling shape of CGiml: X holds the start vectors and comes back with
// the orthonormal Ritz vectors, theta ascending, max_iter and tol are written back (tol: the largest ‖A·x_j − θ_j·x_j‖₂/‖A‖∞), the status is returned
// (0 converged / 1 max_iter / 2 start block rank deficient / 3 trial basis rank deficient or not a number).  M: NULL for none.
inline int LOBPCGiml(const DeviceMatrix &A, std::vector<Vector> &X, std::vector<double> &theta, std::vector<double> &resid, const MultiGridPrecond *M, int &max_iter, double &tol) {
  std::vector<mgs_vec *> x;
  for (Vector &c : X) x.push_back(c.out());
  theta.assign(X.size(), 0.0); resid.assign(X.size(), 0.0);
  int status = -1;
  check(mgs_eig_lobpcg(A.handle(), M && M->use_preconditioner() ? M->handle() : nullptr, (int)x.size(), x.data(), theta.data(), resid.data(), &max_iter, &tol, &status), context());
  return status;
}
inline int LOBPCGiml(const DeviceMatrix &A, std::vector<Vector> &X, std::vector<double> &theta, const MultiGridPrecond &M, int &max_iter, double &tol) {
  std::vector<double> resid;
  return LOBPCGiml(A, X, theta, resid, &M, max_iter, tol);
}
// The generalised problem A·x = λ·B·x, B symmetric positive definite (mgs_eig_lobpcg_gen): X comes back B-orthonormal, tol is the largest
// ‖A·x_j − θ_j·B·x_j‖₂/(‖A‖∞ + |θ_j|·‖B‖∞); status 2 also for a B that XᵀBX shows not to be positive definite.  No declared null space on A or B.
inline int LOBPCGiml(const DeviceMatrix &A, const DeviceMatrix &B, std::vector<Vector> &X, std::vector<double> &theta, std::vector<double> &resid, const MultiGridPrecond *M,
                     int &max_iter, double &tol) {
  std::vector<mgs_vec *> x;
  for (Vector &c : X) x.push_back(c.out());
  theta.assign(X.size(), 0.0); resid.assign(X.size(), 0.0);
  int status = -1;
  check(mgs_eig_lobpcg_gen(A.handle(), B.handle(), M && M->use_preconditioner() ? M->handle() : nullptr, (int)x.size(), x.data(), theta.data(), resid.data(), &max_iter, &tol,
                           &status), context());
  return status;
}
// r = ax − θ·bx, → ‖r‖² with the bits of r.dot(r) (mgs_eig_residual: one pass); r may be ax or bx
inline double eigResidual(const Vector &ax, const Vector &bx, double theta, Vector &r) {
  double s = 0.0;
  check(mgs_eig_residual(context(), r.size(), ax.handle(), bx.handle(), theta, r.out(), &s), context());
  return s;
}

// ---------------------------------------------------------------- projected initial guesses (mgs.h: mgs_guess)
// No reference counterpart: the reference solves one right-hand side (bicg.cpp:159-166).  For a caller who solves with the same operator
// again and again:   SolutionGuess guess(A, MGS_GUESS_ENERGY);   per step:  guess.apply(b, x);  CGiml(A, x, b, M, it, tol);  guess.update(x);
// The guess keeps the DeviceMatrix (and with it the device matrix) alive.  MGS_GUESS_RESIDUAL serves any nonsingular A (BiCGSTABiml).
class SolutionGuess {
  DeviceMatrix A_;
  std::shared_ptr<mgs_guess> g_;
  int64_t info(int i) const { int64_t o[6]; check(mgs_guess_info(g_.get(), o), context()); return o[i]; }
 public:
  SolutionGuess(const DeviceMatrix &A, int kind = MGS_GUESS_ENERGY, int capacity = 8) : A_(A) {
    mgs_guess *p = nullptr;
    check(mgs_guess_create(A.handle(), kind, capacity, &p), context());
    g_ = std::shared_ptr<mgs_guess>(p, [](mgs_guess *q) { mgs_guess_destroy(q); });
  }
  // x0 = projection onto the stored span, enqueued; no host round trip
  void applyAsync(const Vector &b, Vector &x0) { check(mgs_guess_apply(g_.get(), b.handle(), x0.out(), nullptr), context()); }
  // ... and ‖b − A·x0‖/‖b‖ (1 with an empty basis); synchronises
  double apply(const Vector &b, Vector &x0) { double r = 0.0; check(mgs_guess_apply(g_.get(), b.handle(), x0.out(), &r), context()); return r; }
  // offer a solution just computed; false: it lies numerically inside the span (or A is not positive along it) and was not added
  bool update(const Vector &x) { int added = 0; check(mgs_guess_update(g_.get(), x.handle(), &added), context()); return added != 0; }
  void rebase() { check(mgs_guess_rebase(g_.get()), context()); }      // after DeviceMatrix::update_values
  void reset() { check(mgs_guess_reset(g_.get()), context()); }
  int size() const { return (int)info(0); }
  int capacity() const { return (int)info(1); }
  int64_t restarts() const { return info(3); }
  int64_t refused() const { return info(4); }
  mgs_guess *handle() const { return g_.get(); }
};

// ---------------------------------------------------------------- PCG with device-resident scalars (mgs.h: mgs_pcg_plan)
// No reference counterpart for the asynchronous form.  CGiml's arithmetic and bits with one host look per iteration (solve), or none at all
// (enqueue + result).  With SolutionGuess, a time step that never holds the host thread:
//   guess.applyAsync(b, x);  plan.enqueue(x, b, iters, tol);  /* ... other host work ... */  plan.result(it, resid);  guess.update(x);
// The plan keeps the DeviceMatrix and the preconditioner alive.  x and b must stay alive until result() (or a synchronisation).
class PcgPlan {
  DeviceMatrix A_;
  MultiGridPrecond M_;
  std::shared_ptr<mgs_pcg_plan> p_;
 public:
  PcgPlan(const DeviceMatrix &A, const MultiGridPrecond &M) : A_(A), M_(M) {
    mgs_pcg_plan *p = nullptr;
    check(mgs_pcg_plan_create(A.handle(), M.use_preconditioner() ? M.handle() : nullptr, M.symmetric() ? 0 : 1, &p), context());
    p_ = std::shared_ptr<mgs_pcg_plan>(p, [](mgs_pcg_plan *q) { mgs_pcg_plan_destroy(q); });
  }
  // CGiml's contract: returns the status, max_iter and tol are written back; `ahead` iterations stay enqueued beyond the last outcome seen
  int solve(Vector &x, const Vector &b, int &max_iter, double &tol, int ahead = 1) {
    int status = -1;
    check(mgs_pcg_plan_solve(p_.get(), x.out(), b.handle(), ahead, &max_iter, &tol, &status), context());
    return status;
  }
  // INIT, `iters` iterations and the final true residual, enqueued; no host wait
  void enqueue(Vector &x, const Vector &b, int iters, double tol) { check(mgs_pcg_plan_enqueue(p_.get(), x.out(), b.handle(), iters, tol), context()); }
  // of the last enqueue (synchronises): returns the status; iterations done and the true relative residual
  int result(int &iters_done, double &resid) {
    int status = -1;
    check(mgs_pcg_plan_result(p_.get(), &iters_done, &resid, &status), context());
    return status;
  }
  int64_t info(int i) const { int64_t o[6]; check(mgs_pcg_plan_info(p_.get(), o), context()); return o[i]; }
  mgs_pcg_plan *handle() const { return p_.get(); }
};

// ---------------------------------------------------------------- BiCGSTAB with device-resident scalars (mgs.h: mgs_bicgstab_plan)
// bicg.cpp:74-136 has no asynchronous form.  BiCGSTABiml's arithmetic and bits with one host look per iteration (solve), or none at all
// (enqueue + result, which also reports the true residual bicg.cpp never forms).  With SolutionGuess(A, MGS_GUESS_RESIDUAL):
//   guess.applyAsync(b, x);  plan.enqueue(x, b, iters, tol);  /* ... other host work ... */  plan.result(it, resid);  guess.update(x);
// The plan keeps the DeviceMatrix and the preconditioner alive.  x and b must stay alive until result() (or a synchronisation).
class BicgstabPlan {
  DeviceMatrix A_;
  MultiGridPrecond M_;
  std::shared_ptr<mgs_bicgstab_plan> p_;
 public:
  BicgstabPlan(const DeviceMatrix &A, const MultiGridPrecond &M) : A_(A), M_(M) {
    mgs_bicgstab_plan *p = nullptr;
    check(mgs_bicgstab_plan_create(A.handle(), M.use_preconditioner() ? M.handle() : nullptr, &p), context());
    p_ = std::shared_ptr<mgs_bicgstab_plan>(p, [](mgs_bicgstab_plan *q) { mgs_bicgstab_plan_destroy(q); });
  }
  // BiCGSTABiml's contract: returns the status, max_iter and tol are written back; `ahead` iterations stay enqueued beyond the last outcome seen
  int solve(Vector &x, const Vector &b, int &max_iter, double &tol, int ahead = 1) {
    int status = -1;
    check(mgs_bicgstab_plan_solve(p_.get(), x.out(), b.handle(), ahead, &max_iter, &tol, &status), context());
    return status;
  }
  // INIT, `iters` iterations and the final true residual, enqueued; no host wait
  void enqueue(Vector &x, const Vector &b, int iters, double tol) { check(mgs_bicgstab_plan_enqueue(p_.get(), x.out(), b.handle(), iters, tol), context()); }
  // of the last enqueue (synchronises): returns the status; iterations done, the true relative residual and (optionally) the recursion's
  int result(int &iters_done, double &resid, double *recursive_resid = nullptr) {
    int status = -1;
    check(mgs_bicgstab_plan_result(p_.get(), &iters_done, &resid, recursive_resid, &status), context());
    return status;
  }
  int64_t info(int i) const { int64_t o[6]; check(mgs_bicgstab_plan_info(p_.get(), o), context()); return o[i]; }
  mgs_bicgstab_plan *handle() const { return p_.get(); }
};

// ---------------------------------------------------------------- flexible GCR with device-resident coefficients (mgs.h: mgs_fgcr_plan)
// The reference has no flexible method (nearest line: src/CPU_Matlab/solve.m:28-33) and no asynchronous form.  mgs_fgcr's arithmetic and bits —
// the Krylov method the K-cycle needs on nonsymmetric operators — with one host look per iteration (solve), or none at all (enqueue + result):
//   guess.applyAsync(b, x);  plan.enqueue(x, b, iters, tol);  /* ... other host work ... */  plan.result(it, resid);  guess.update(x);
// The plan keeps the DeviceMatrix and the preconditioner alive.  x and b must stay alive until result() (or a synchronisation).
class FgcrPlan {
  DeviceMatrix A_;
  MultiGridPrecond M_;
  std::shared_ptr<mgs_fgcr_plan> p_;
 public:
  FgcrPlan(const DeviceMatrix &A, const MultiGridPrecond &M, int restart = 10) : A_(A), M_(M) {      // restart in 1..16
    mgs_fgcr_plan *p = nullptr;
    check(mgs_fgcr_plan_create(A.handle(), M.use_preconditioner() ? M.handle() : nullptr, restart, &p), context());
    p_ = std::shared_ptr<mgs_fgcr_plan>(p, [](mgs_fgcr_plan *q) { mgs_fgcr_plan_destroy(q); });
  }
  // mgs_fgcr's contract: returns the status, max_iter and tol are written back; `ahead` iterations stay enqueued beyond the last outcome seen
  // (0 by default: with a K-cycle the iteration that ahead = 1 runs frozen costs more than the look it hides, profiles/r14_fgcr_plan.md)
  int solve(Vector &x, const Vector &b, int &max_iter, double &tol, int ahead = 0) {
    int status = -1;
    check(mgs_fgcr_plan_solve(p_.get(), x.out(), b.handle(), ahead, &max_iter, &tol, &status), context());
    return status;
  }
  // INIT, `iters` iterations with their scheduled window closes and the final true residual, enqueued; no host wait
  void enqueue(Vector &x, const Vector &b, int iters, double tol) { check(mgs_fgcr_plan_enqueue(p_.get(), x.out(), b.handle(), iters, tol), context()); }
  // of the last enqueue (synchronises): returns the status; iterations done, the true relative residual and (optionally) the recursion's
  int result(int &iters_done, double &resid, double *recursive_resid = nullptr) {
    int status = -1;
    check(mgs_fgcr_plan_result(p_.get(), &iters_done, &resid, recursive_resid, &status), context());
    return status;
  }
  int64_t info(int i) const { int64_t o[6]; check(mgs_fgcr_plan_info(p_.get(), o), context()); return o[i]; }
  mgs_fgcr_plan *handle() const { return p_.get(); }
};

// ---------------------------------------------------------------- MINRES with device-resident scalars (mgs.h: mgs_minres_plan)
// The reference has no MINRES (nearest line: src/CPU_Matlab/solve.m:28-33) and no asynchronous form.  mgs_minres's arithmetic and bits — symmetric
// indefinite systems with a V(nu, nu) preconditioner — with one host look per iteration instead of two (solve), or none at all (enqueue + result):
//   D.update_values_coo(v, nt);  Dt.transposeUpdate(D);  K.bmatUpdate(2, 2, blocks);  M.refresh();  plan.enqueue(x, b, iters, tol);  plan.result(it, resid);
// There is no recalibration on the device: result() == 1 with it < iters means the estimate ran ahead of the 2-norm; enqueue again from x.
// The plan keeps the DeviceMatrix and the preconditioner alive.  x and b must stay alive until result() (or a synchronisation).
class MinresPlan {
  DeviceMatrix A_;
  MultiGridPrecond M_;
  std::shared_ptr<mgs_minres_plan> p_;
 public:
  MinresPlan(const DeviceMatrix &A, const MultiGridPrecond &M) : A_(A), M_(M) {
    mgs_minres_plan *p = nullptr;
    check(mgs_minres_plan_create(A.handle(), M.use_preconditioner() ? M.handle() : nullptr, &p), context());
    p_ = std::shared_ptr<mgs_minres_plan>(p, [](mgs_minres_plan *q) { mgs_minres_plan_destroy(q); });
  }
  // mgs_minres's contract: returns the status, max_iter and tol (the true relative residual) are written back; `ahead` iterations stay enqueued
  // beyond the last outcome seen
  int solve(Vector &x, const Vector &b, int &max_iter, double &tol, int ahead = 1) {
    int status = -1;
    check(mgs_minres_plan_solve(p_.get(), x.out(), b.handle(), ahead, &max_iter, &tol, &status), context());
    return status;
  }
  // INIT, `iters` iterations and the final true residual, enqueued; no host wait
  void enqueue(Vector &x, const Vector &b, int iters, double tol) { check(mgs_minres_plan_enqueue(p_.get(), x.out(), b.handle(), iters, tol), context()); }
  // of the last enqueue (synchronises): returns the status; iterations done, the true relative residual and (optionally) the estimate
  int result(int &iters_done, double &resid, double *recursive_resid = nullptr) {
    int status = -1;
    check(mgs_minres_plan_result(p_.get(), &iters_done, &resid, recursive_resid, &status), context());
    return status;
  }
  int64_t info(int i) const { int64_t o[6]; check(mgs_minres_plan_info(p_.get(), o), context()); return o[i]; }
  mgs_minres_plan *handle() const { return p_.get(); }
};

// ---------------------------------------------------------------- TicToc.cpp:18-53
class TicToc {
  std::chrono::time_point<std::chrono::system_clock> start;
  std::string s; int level;
 public:
  TicToc(std::string s_, int level_) : s(s_), level(level_) {}
  void tic() { start = std::chrono::system_clock::now(); }
  double toc() {
    mgs_sync(context());
    std::chrono::duration<float> diff = std::chrono::system_clock::now() - start;
    std::string line = "\033[1;34m[time] \033[0m" + s;
    for (int i = 0; i < level; i++) fprintf(stderr, " ");
    while (line.size() < 60) line += ' ';
    fprintf(stderr, "%s : %lf.\n", line.c_str(), diff.count());
    return diff.count();
  }
};
template <typename T> void printScreen(const int level, std::string s, const T tm) {
  for (int i = 0; i < level; i++) std::cout << " ";
  std::cout << "\033[32m\033[1m[info] \033[00m";
  while (s.size() + 18 < 60) s += ' ';
  std::cout << s << " : " << tm << ".\n";
}

}  // namespace mgs
