// What the programs of tests/cpp_face share: raw little-endian files in, raw files and one table of scalars out (tests/cpp_face.py reads
// them back), and index lists placed in device memory through an mgs::Vector — mgs_host.hpp offers no raw allocation and this needs no HIP header.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "mgs_host.hpp"

namespace face {

template <typename T> std::vector<T> read_raw(const std::string &path) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) throw std::runtime_error("cannot open " + path);
  const std::streamsize bytes = f.tellg();
  f.seekg(0);
  std::vector<T> a((size_t)bytes / sizeof(T));
  if (bytes) f.read((char *)a.data(), bytes);
  return a;
}
template <typename T> void write_raw(const std::string &path, const std::vector<T> &a) {
  std::ofstream f(path, std::ios::binary);
  if (!a.empty()) f.write((const char *)a.data(), (std::streamsize)(a.size() * sizeof(T)));
  if (!f) throw std::runtime_error("cannot write " + path);
}

// an index list (or any other plain array) in device memory: its bytes inside a Vector of doubles
template <typename T> struct DevList {
  mgs::Vector store;
  int64_t n = 0;
  explicit DevList(const std::vector<T> &a) : store((int64_t)((a.size() * sizeof(T) + 7) / 8 + 1)), n((int64_t)a.size()) {
    std::vector<double> h((size_t)store.size(), 0.0);
    if (!a.empty()) std::memcpy(h.data(), a.data(), a.size() * sizeof(T));
    store.upload(h);
  }
  const void *ptr() const { return mgs_vec_ptr(store.handle()); }
};
inline std::vector<int64_t> widen(const std::vector<int32_t> &a) { return std::vector<int64_t>(a.begin(), a.end()); }

struct Out {
  std::string dir;
  FILE *table;
  explicit Out(const std::string &d) : dir(d), table(std::fopen((d + "/scalars.txt").c_str(), "w")) {
    if (!table) throw std::runtime_error("cannot write " + d + "/scalars.txt");
  }
  ~Out() { if (table) std::fclose(table); }
  Out(const Out &) = delete;
  Out &operator=(const Out &) = delete;
  void count(const std::string &name, long long v) { std::fprintf(table, "%s i %lld\n", name.c_str(), v); std::fflush(table); }
  void number(const std::string &name, double v) { std::fprintf(table, "%s d %a\n", name.c_str(), v); std::fflush(table); }
  void f64(const std::string &name, const std::vector<double> &a) { write_raw(dir + "/" + name + ".f64", a); }
  void vec(const std::string &name, const mgs::Vector &v) { f64(name, v.download()); }
  // every array of a device matrix, the shape the wrapper caches and the shape the library holds
  void csr(const std::string &name, const mgs::DeviceMatrix &M) {
    int r = 0, c = 0; int64_t nnz = 0;
    mgs::check(mgs_csr_shape(M.handle(), &r, &c, &nnz), mgs::context());
    std::vector<int> rp((size_t)r + 1), ci((size_t)nnz + 1);
    std::vector<double> v((size_t)nnz + 1);
    mgs::check(mgs_csr_download(M.handle(), rp.data(), ci.data(), v.data()), mgs::context());
    ci.resize((size_t)nnz); v.resize((size_t)nnz);
    write_raw(dir + "/" + name + ".rp.i32", rp); write_raw(dir + "/" + name + ".ci.i32", ci); f64(name + ".val", v);
    count(name + ".rows", M.rows()); count(name + ".cols", M.cols());
    count(name + ".lib_rows", r); count(name + ".lib_cols", c);
  }
};

inline mgs::Vector load_vec(const std::string &path) {
  std::vector<double> h = read_raw<double>(path);
  mgs::Vector v((int64_t)h.size());
  v.upload(h);
  return v;
}

// main() of every program: usage without touching a device, and an exception ends the program with status 3 and its text
template <typename F> int run(int argc, char **argv, F body) {
  if (argc != 3) { std::cout << "usage: " << (argc ? argv[0] : "program") << " IN_DIR OUT_DIR" << std::endl; return 1; }
  try {
    Out out(argv[2]);
    body(std::string(argv[1]) + "/", out);
  } catch (const std::exception &e) {
    std::cout << "EXCEPTION " << e.what() << std::endl;
    return 3;
  }
  return 0;
}

}  // namespace face
