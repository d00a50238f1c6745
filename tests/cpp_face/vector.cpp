// mgs::Vector and its host mirror.  In: a.f64, b.f64 (integer-valued), c.f64, d.f64 (any values), all of one length.
#include "face_io.hpp"
using namespace mgs;

int main(int argc, char **argv) {
  return face::run(argc, argv, [](const std::string &in, face::Out &out) {
    const std::vector<double> a = face::read_raw<double>(in + "a.f64"), b = face::read_raw<double>(in + "b.f64");
    const int64_t n = (int64_t)a.size();
    Vector va(n), vb(n);
    va.upload(a); vb.upload(b);

    {  // element writes, then a device operation
      Vector v(n); v.upload(a);
      v[3] = 7.0; v(n - 1) = -2.0;
      Vector w = v + vb;
      out.vec("write_then_op", w);
    }
    {  // a device operation, then element reads: the mirror taken before it is stale
      Vector v(n); v.upload(a);
      out.number("read_before_op", v[0]);
      v += vb;
      out.number("read_after_op", v[0]);
      const Vector &cv = v;
      out.number("read_after_op_const", cv(n - 2));
      out.vec("op_then_read", v);
    }
    {  // a copy sees the writes
      Vector v(n); v.upload(a);
      v[1] = 99.0;
      Vector c(v);
      out.vec("copy_construct", c);
      c[2] = -5.0;                                  // and is deep
      out.vec("copy_construct_source", v);
      out.vec("copy_construct_written", c);
    }
    {  // copy-assign over a vector whose mirror is valid and dirty
      Vector t(n); t.upload(b);
      t[2] = 5.0;
      t = va;
      out.number("copy_assign_read", t[2]);
      out.vec("copy_assign", t);
      Vector s(n); s.upload(b);
      s[4] = 6.0;
      Vector &alias = s;
      s = alias;                                    // self-assignment keeps the pending write
      out.vec("self_assign", s);
    }
    {  // moves of a dirty vector
      Vector m(n); m.upload(a);
      m[4] = -8.0;
      Vector mm(std::move(m));
      out.vec("move_construct", mm);
      Vector q(n); q.upload(b);
      q[0] = 11.0;
      Vector z(n); z.setZero();
      z[1] = 3.0;
      z = std::move(q);
      out.number("move_assign_read", z[0]);
      out.vec("move_assign", z);
    }
    {  // x += x with a pending write
      Vector s(n); s.upload(a);
      s[0] = 4.0;
      s += s;
      out.vec("self_add", s);
      s -= s;
      out.vec("self_sub", s);
    }
    {  // setZero / upload after element writes: the pending writes do not come back
      Vector u(n); u.upload(a);
      u[3] = 5.0;
      u.setZero();
      out.vec("set_zero_after_write", u);
      out.number("set_zero_read", u[3]);
      const Vector &cu = u;
      (void)cu[2];
      u[2] = 9.0;
      u.upload(b);
      out.vec("upload_after_write", u);
      u += va;
      out.vec("upload_after_write_then_op", u);
    }
    {  // operator[] const after out()
      Vector k(n); k.upload(a);
      const Vector &ck = k;
      out.number("const_read_before", ck[2]);
      k.upload(b);
      out.number("const_read_after_upload", ck[2]);
      k.setZero();
      out.number("const_read_after_zero", ck[2]);
      check(mgs_vec_copy(va.handle(), k.out()), context());
      out.number("const_read_after_out", ck[2]);
    }
    {  // download() with pending writes
      Vector d(n); d.upload(a);
      d[6] = 42.0;
      out.f64("download_pending", d.download());
    }
    {  // no entries
      Vector e(0), none;
      out.count("empty_size", e.size()); out.count("none_size", none.size());
      out.count("empty_download", (long long)e.download().size());
      Vector ec(e);
      out.count("empty_copy_size", ec.size());
      e.setZero();
      Vector nc(none);
      out.count("none_copy_size", nc.rows());
    }
    {  // arithmetic, on values that round
      Vector c = face::load_vec(in + "c.f64"), d = face::load_vec(in + "d.f64");
      out.vec("plus", c + d);
      out.vec("minus", c - d);
      out.vec("scaled_left", 2.5 * c);
      out.vec("scaled_right", d * -0.3);
      Vector p = c; p += d;
      out.vec("plus_assign", p);
      Vector m = c; m -= d;
      out.vec("minus_assign", m);
      out.vec("chain", c + 0.7 * d - 1.1 * (c - d));
      out.number("dot", c.dot(d)); out.number("dot_free", dot(d, c));
      out.number("norm", c.norm()); out.number("norm_free", norm(d));
      out.number("dot_int", va.dot(vb));
    }
  });
}
