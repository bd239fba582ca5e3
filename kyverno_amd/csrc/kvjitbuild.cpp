// Specialized kernels for a compiled policy set (see kvjit.hpp): from the generated programs
// (kvjitgen.cpp) to the final kernels' code objects. The code-object cache and the hiprtc /
// child-process compiles, the register plan (block probes, the spill ladder, one register
// verdict for all of them), the output-mode variants, the plan cache, and jit_build, the
// order in which they run.
#include <hip/hiprtc.h>

#include <dlfcn.h>
#include <sched.h>
#include <spawn.h>
#include <sys/stat.h>
#include <sys/wait.h>

#include <cerrno>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <sstream>
#include <stdexcept>
#include <thread>

#include "kvjit.hpp"

extern char** environ;

namespace kvh {

using namespace kv;

namespace {

uint64_t fnv1a64(const std::string& a, uint64_t h = 1469598103934665603ull) {
  for (unsigned char c : a) h = (h ^ c) * 1099511628211ull;
  return h;
}

std::string cache_dir() {
  const char* e = getenv("KVGPU_JIT_CACHE");
  if (e && std::string(e) == "0") return "";
  if (e && *e) return e;
  if (const char* x = getenv("XDG_CACHE_HOME"); x && *x) return std::string(x) + "/kvgpu";
  if (const char* h = getenv("HOME"); h && *h) return std::string(h) + "/.cache/kvgpu";
  return "";
}

bool read_file(const std::string& path, std::vector<char>* out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  out->resize(n > 0 ? (size_t)n : 0);
  const bool ok = n > 0 && fread(out->data(), 1, (size_t)n, f) == (size_t)n;
  fclose(f);
  return ok;
}

template <class Buf>  // (a string or a vector of char)
bool write_file(const std::string& path, const Buf& data) {
  FILE* f = fopen(path.c_str(), "wb");
  const bool ok = f && fwrite(data.data(), 1, data.size(), f) == data.size();
  if (f) fclose(f);
  return ok;
}

template <class Buf>
void write_file_atomic(const std::string& dir, const std::string& path, const Buf& data) {
  std::string cmd = dir;  // create the directory (one level under an existing parent is enough here)
  for (size_t i = 1; i <= cmd.size(); i++)
    if (i == cmd.size() || cmd[i] == '/') mkdir(cmd.substr(0, i).c_str(), 0755);
  const std::string tmp = path + ".tmp." + std::to_string((unsigned long long)getpid()) + "." +
                          std::to_string(std::hash<std::thread::id>()(std::this_thread::get_id()));
  if (!write_file(tmp, data) || rename(tmp.c_str(), path.c_str()) != 0) unlink(tmp.c_str());
}

const char* const kOpts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-label", "-Wno-unused-variable"};
std::vector<char> compile_one(const std::string& src, const std::string& name) {
  hiprtcProgram prog;
  if (hiprtcCreateProgram(&prog, src.c_str(), (name + ".hip").c_str(), 0, nullptr, nullptr) != HIPRTC_SUCCESS)
    throw std::runtime_error("hiprtcCreateProgram failed");
  if (hiprtcCompileProgram(prog, (int)(sizeof kOpts / sizeof kOpts[0]), kOpts) != HIPRTC_SUCCESS) {
    size_t ls = 0;
    hiprtcGetProgramLogSize(prog, &ls);
    std::string log(ls, '\0');
    if (ls) hiprtcGetProgramLog(prog, &log[0]);
    hiprtcDestroyProgram(&prog);
    throw std::runtime_error("hiprtc compile of " + name + " failed: " + log.substr(0, 4000));
  }
  size_t cs = 0;
  hiprtcGetCodeSize(prog, &cs);
  std::vector<char> code(cs);
  hiprtcGetCode(prog, code.data());
  hiprtcDestroyProgram(&prog);
  return code;
}

// kvjitc next to libkvgpu.so (KVGPU_JITC overrides): compiles one program per process
std::string jitc_path() {
  if (const char* e = getenv("KVGPU_JITC")) return e;
  Dl_info info{};
  if (!dladdr((void*)&jitc_path, &info) || !info.dli_fname) return "";
  std::string p = info.dli_fname;
  const size_t slash = p.rfind('/');
  p = (slash == std::string::npos ? std::string(".") : p.substr(0, slash)) + "/kvjitc";
  return access(p.c_str(), X_OK) == 0 ? p : "";
}

// cores this process may use: affinity, capped by a cgroup v2 CPU quota
unsigned host_threads() {
  unsigned n = std::thread::hardware_concurrency();
  cpu_set_t cs;
  if (sched_getaffinity(0, sizeof cs, &cs) == 0) n = (unsigned)CPU_COUNT(&cs);
  if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[32] = {0};
    unsigned long long per = 0;
    if (fscanf(f, "%31s %llu", q, &per) == 2 && strcmp(q, "max") != 0 && per)
      n = std::min<unsigned>(n, (unsigned)std::max(1ull, strtoull(q, nullptr, 10) / per));
    fclose(f);
  }
  return std::max(1u, n);
}

// compile programs `todo` of img in child processes (kvjitc), `T` at a time
void compile_in_children(JitImage* img, const std::vector<size_t>& todo, const std::string& jitc, unsigned T) {
  const char* td = getenv("TMPDIR");
  std::string dir = std::string(td && *td ? td : "/tmp") + "/kvjit.XXXXXX";
  if (!mkdtemp(&dir[0])) throw std::runtime_error("kvjit: mkdtemp failed");
  std::atomic<size_t> next{0}, done{0};
  std::vector<std::string> errs(T);
  // KVGPU_PROGRESS=1: a line on stderr at most every 15 s (long compiles stay visibly alive)
  const bool progress = getenv("KVGPU_PROGRESS") && getenv("KVGPU_PROGRESS")[0] == '1';
  const auto t0 = std::chrono::steady_clock::now();
  std::atomic<int64_t> last_ms{0};
  std::vector<std::thread> th;
  for (unsigned t = 0; t < T; t++)
    th.emplace_back([&, t]() {
      for (size_t j; (j = next++) < todo.size();) {
        const size_t i = todo[j];
        const std::string src = dir + "/" + std::to_string(i) + ".hip", out = dir + "/" + std::to_string(i) + ".co";
        if (!write_file(src, img->common + img->kernel_src[i])) {
          errs[t] = "kvjit: cannot write " + src;
          return;
        }
        std::string av[] = {jitc, src, out, img->kernel_name[i]};
        char* const argv[] = {&av[0][0], &av[1][0], &av[2][0], &av[3][0], nullptr};
        pid_t pid = 0;
        if (posix_spawn(&pid, jitc.c_str(), nullptr, nullptr, argv, environ) != 0) {
          errs[t] = "kvjit: cannot start " + jitc;
          return;
        }
        int status = 0;
        while (waitpid(pid, &status, 0) < 0 && errno == EINTR) continue;
        if (!WIFEXITED(status) || WEXITSTATUS(status) != 0 || !read_file(out, &img->codes[i])) {
          errs[t] = "kvjit: compiling " + img->kernel_name[i] + " failed (kvjitc status " + std::to_string(status) + ")";
          return;
        }
        unlink(src.c_str());
        unlink(out.c_str());
        const size_t d = ++done;
        if (progress) {
          const int64_t now =
              (int64_t)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
          int64_t prev = last_ms.load();
          if (now - prev >= 15000 && last_ms.compare_exchange_strong(prev, now))
            fprintf(stderr, "[kvgpu] hiprtc: %zu/%zu kernel programs compiled (%.0f s)\n", d, todo.size(), now / 1e3);
        }
      }
    });
  for (auto& x : th) x.join();
  rmdir(dir.c_str());
  for (auto& e : errs)
    if (!e.empty()) throw std::runtime_error(e);
}

// Private (scratch) segment size and VGPR count of kernel `name` in a gfx950 code object,
// from the kernel descriptor `<name>.kd` (offset 4: private_segment_fixed_size); false when
// the object lacks the descriptor or the function symbol. A non-zero private segment in these
// kernels means register spills (they keep no arrays on the stack).
bool co_kernel_info(const std::vector<char>& co, const std::string& name, uint32_t* private_seg, uint32_t* vgprs) {
  auto rd = [&](size_t off, size_t n, void* out) {
    if (off + n > co.size()) return false;
    memcpy(out, co.data() + off, n);
    return true;
  };
  if (co.size() < 64 || memcmp(co.data(), "\x7f" "ELF", 4) != 0 || co[4] != 2) return false;
  uint64_t shoff = 0;
  uint16_t shentsize = 0, shnum = 0;
  rd(0x28, 8, &shoff);
  rd(0x3A, 2, &shentsize);
  rd(0x3C, 2, &shnum);
  struct Sh { uint32_t name, type; uint64_t flags, addr, off, size; uint32_t link, info; uint64_t align, entsize; };
  std::vector<Sh> sh(shnum);
  for (uint16_t i = 0; i < shnum; i++)
    if (!rd(shoff + (uint64_t)i * shentsize, sizeof(Sh), &sh[i])) return false;
  bool kd = false, fn = false;
  for (const Sh& t : sh) {
    if (t.type != 2 /* SHT_SYMTAB */ || t.link >= shnum) continue;
    const Sh& strtab = sh[t.link];
    for (uint64_t o = t.off; o + 24 <= t.off + t.size; o += 24) {
      uint32_t nm = 0;
      uint16_t shndx = 0;
      uint64_t value = 0;
      rd(o, 4, &nm);
      rd(o + 6, 2, &shndx);
      rd(o + 8, 8, &value);
      if (strtab.off + nm >= co.size()) continue;
      const char* sn = co.data() + strtab.off + nm;
      const size_t maxlen = co.size() - (strtab.off + nm);
      const std::string sym(sn, strnlen(sn, maxlen));
      if (sym == name + ".kd" && shndx < shnum) {
        const Sh& sec = sh[shndx];
        kd = rd(sec.off + (value - sec.addr) + 4, 4, private_seg);
        // compute_pgm_rsrc1 (descriptor offset 48): granulated VGPR count, 8-register granules
        // of the unified (arch + acc) file on gfx950
        uint32_t rsrc1 = 0;
        if (kd && rd(sec.off + (value - sec.addr) + 48, 4, &rsrc1)) *vgprs = ((rsrc1 & 0x3Fu) + 1u) * 8u;
      } else if (sym == name) {
        fn = true;
      }
    }
  }
  return kd && fn;
}

// hash of the compiler options, hiprtc version and the common prelude of an image's programs
uint64_t common_hash(const std::string& common) {
  std::string opt_key;
  for (const char* o : kOpts) opt_key += std::string(o) + "\n";
  int hv = 0;
  (void)hiprtcVersion(&hv, &hv);
  opt_key += "hiprtc " + std::to_string(hv) + "\n";
  return fnv1a64(common, fnv1a64(opt_key));
}

// code-object cache file of kernel program i: <name>-<hash of options + program text>.co
std::string cache_file(const JitImage& img, size_t i, uint64_t hcommon) {
  char key[40];
  snprintf(key, sizeof key, "%016llx", (unsigned long long)fnv1a64(img.kernel_src[i], hcommon));
  return img.kernel_name[i] + "-" + key + ".co";
}

// Compile every kernel program with hiprtc for gfx950, on parallel host threads (KVGPU_JIT_THREADS,
// default: hardware threads), through the code-object cache (KVGPU_JIT_CACHE directory, default
// $XDG_CACHE_HOME/kvgpu or ~/.cache/kvgpu; "0" disables; entries keyed by a hash of compiler options
// + program text). Throws std::runtime_error with the log on failure. Adds its time to
// img->compile_ms, as every build step does (a probe or variant image starts at 0; its owner adds it on).
void jit_compile(JitImage* img) {
  auto t0 = std::chrono::steady_clock::now();
  const size_t K = img->kernel_src.size();
  img->codes.assign(K, {});
  const std::string dir = cache_dir();
  const uint64_t hcommon = common_hash(img->common);
  // cache lookups; the misses compile in child processes (hiprtc serialises the
  // compilations of one process), or in this process when kvjitc is unavailable
  // (KVGPU_JIT_PROCS=0 forces that)
  std::vector<std::string> paths(K);
  std::vector<size_t> todo;
  for (size_t i = 0; i < K; i++) {
    paths[i] = dir.empty() ? "" : dir + "/" + cache_file(*img, i, hcommon);
    if (paths[i].empty() || !read_file(paths[i], &img->codes[i])) todo.push_back(i);
  }
  unsigned T = std::min(16u, host_threads());
  if (const char* e = getenv("KVGPU_JIT_THREADS")) T = (unsigned)std::max(1, atoi(e));
  T = std::max(1u, std::min<unsigned>(T, (unsigned)todo.size()));
  const std::string jitc = jitc_path();
  const bool procs = !(getenv("KVGPU_JIT_PROCS") && getenv("KVGPU_JIT_PROCS")[0] == '0');
  if (!todo.empty() && procs && !jitc.empty() && todo.size() > 1) {
    compile_in_children(img, todo, jitc, T);
  } else {
    for (size_t i : todo) img->codes[i] = compile_one(img->common + img->kernel_src[i], img->kernel_name[i]);
  }
  if (!dir.empty())
    for (size_t i : todo) write_file_atomic(dir, paths[i], img->codes[i]);
  img->compile_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// the program (index into kernel_name / kernel_src / codes) of kernel `name`; none: kernel_name.size()
size_t program_of(const JitImage& img, const std::string& name) {
  return (size_t)(std::find(img.kernel_name.begin(), img.kernel_name.end(), name) - img.kernel_name.begin());
}

// The verdict of compiled program `ci` of img under a bound of `waves`, from its kernel
// descriptor; false when there is no such program or descriptor.
bool reg_verdict(const JitImage& img, size_t ci, int waves, RegVerdict* out) {
  uint32_t priv = 0, vgprs = 0;
  if (ci >= img.codes.size() || !co_kernel_info(img.codes[ci], img.kernel_name[ci], &priv, &vgprs)) return false;
  *out = reg_verdict_of(priv, vgprs, waves, img.kernel_src[ci].find("kv_dleaf_impl") != std::string::npos);
  return true;
}

// common of the output-mode variant `full` of img's programs (also what names their cache files)
std::string variant_common(const JitImage& img, uint32_t full) {
  return "#define KVJ_FULL " + std::to_string(full) + "u\n" + img.common;
}

}  // namespace

RegVerdict reg_verdict_of(uint32_t priv, uint32_t vgprs, int waves, bool calls) {
  RegVerdict v{priv, vgprs, calls, false, false};
  v.fits = waves == 0 || vgprs <= 512u / (uint32_t)waves;
  v.scratch_ok = priv == 0 || (calls && waves == 0);
  return v;
}

bool jit_plan_spills(JitImage* img, const std::vector<RegVerdict>& verdicts) {
  // (DESIGN.md §4 *Register plan*: every faulting round-1 build had a private segment)
  std::vector<JitKernelPlan> next;
  bool changed = false;
  for (size_t k = 0; k < img->plan.size(); k++) {
    const JitKernelPlan& kp = img->plan[k];
    const RegVerdict& v = verdicts.at(k);
    if (v.ships()) {
      next.push_back(kp);
      continue;
    }
    changed = true;
    JitKernelPlan np = kp;
    const size_t big = (size_t)(std::max_element(np.blocks.begin(), np.blocks.end()) - np.blocks.begin());  // (the first)
    if (kp.colloops) {  // (the plan comes first: the column loops go, then the three-part layout, before a block or a wave does)
      np.colloops = false;
    } else if (kp.grouped) {
      np.grouped = false;
    } else if (v.calls && v.fits) {  // (its scratch is the call frame: it drops its bound instead of splitting blocks)
      np.waves = 0;
    } else if (kp.waves > 6 && np.blocks.size() > 1) {
      // the blocks met the bound alone (jit_refine_blocks) and the kernel still does not: the
      // pressure crosses blocks, which splitting one block at a time fixes only slowly (C4:
      // 20+ recompiles); a kernel of multi-block form gives up a wave first (down to 6)
      np.waves = kp.waves - 1;
    } else if (!np.blocks.empty() && np.blocks[big] > 1) {  // the largest block in two halves
      const uint32_t c = np.blocks[big], h = c / 2;
      np.blocks[big] = h;
      np.blocks.insert(np.blocks.begin() + big + 1, c - h);
    } else if (kp.waves > 1) {
      np.waves = kp.waves - 1;
    } else if (kp.waves == 1) {
      np.waves = 0;
    } else if (kp.count > 1) {
      const uint32_t h = kp.count / 2;
      next.push_back({kp.first, h, 0, std::vector<uint32_t>(h, 1u)});
      next.push_back({kp.first + h, kp.count - h, 0, std::vector<uint32_t>(kp.count - h, 1u)});
      continue;
    } else {
      throw std::runtime_error("kvjit: kernel " + img->chunks[k].name + " needs " + std::to_string(v.priv) +
                               " B of scratch per lane even without a launch bound");
    }
    next.push_back(np);
  }
  if (changed) img->plan = next;
  return changed;
}

namespace {

// The re-plan step over the compiled image: the verdict of every planned kernel, then the ladder.
bool jit_plan_spills(JitImage* img) {
  std::vector<RegVerdict> verdicts(img->plan.size());
  for (size_t k = 0; k < img->plan.size(); k++)
    if (!reg_verdict(*img, program_of(*img, img->chunks[k].name), img->plan[k].waves, &verdicts[k]))
      throw std::runtime_error("kvjit: no kernel descriptor for " + img->chunks[k].name);
  return jit_plan_spills(img, verdicts);
}

// The output-mode variants of the final plan (JitImage::variants): FULL (status + records, DevOut::
// full 3) and SCOPES-only (per-scope counts, 8); through the code-object cache.
void jit_compile_variants(JitImage* img) {
  img->variants.clear();
  for (uint32_t full : {3u, 8u}) {
    JitImage v;
    v.common = variant_common(*img, full);
    std::vector<size_t> at;  // program of each variant program
    for (size_t i = 0; i < img->kernel_name.size(); i++)
      if (img->kernel_name[i].rfind("kvj_r", 0) == 0) {
        v.kernel_name.push_back(img->kernel_name[i]);
        v.kernel_src.push_back(img->kernel_src[i]);
        at.push_back(i);
      }
    if (at.empty()) return;
    jit_compile(&v);
    img->compile_ms += v.compile_ms;
    JitImage::Variant out;
    out.full = full;
    out.codes.resize(img->kernel_name.size());
    // a variant ships only where it meets the register rules of the generic kernel under the
    // plan's bound of that kernel (a variant without a descriptor does not ship)
    for (size_t k = 0; k < img->chunks.size() && k < img->plan.size(); k++) {
      const size_t j = program_of(v, img->chunks[k].name);
      RegVerdict rv;
      if (reg_verdict(v, j, img->plan[k].waves, &rv) && rv.ships()) out.codes[at[j]] = std::move(v.codes[j]);
    }
    img->variants.push_back(std::move(out));
  }
}

// Block sizes of the plan from probe compiles: every multi-rule block of a multi-block kernel
// is compiled alone as a probe kernel under its kernel's bound (small programs, compiled in
// parallel); a block whose probe spills or exceeds the bound's registers is split in two, and its
// halves are probed in the next round, until every probe meets its bound (then regenerate the image).
void jit_refine_blocks(const PolicySet& ps, uint32_t chunk_rules, JitImage* img) {
  for (int round = 0; round < 12; round++) {
    JitImage probe;
    probe.probe = true;
    probe.col_use = img->col_use;
    std::vector<std::pair<size_t, size_t>> at;  // (kernel, block) of each probe
    for (size_t k = 0; k < img->plan.size(); k++) {
      const JitKernelPlan& kp = img->plan[k];
      if (kp.blocks.size() < 2 || kp.waves == 0) continue;
      uint32_t first = kp.first;
      for (size_t b = 0; b < kp.blocks.size(); b++) {
        if (kp.blocks[b] > 1) {
          probe.plan.push_back({first, kp.blocks[b], kp.waves, {kp.blocks[b]}});
          at.push_back({k, b});
        }
        first += kp.blocks[b];
      }
    }
    if (probe.plan.empty()) return;
    jit_generate(ps, chunk_rules, &probe);
    jit_compile(&probe);
    img->compile_ms += probe.compile_ms;
    std::set<std::pair<size_t, size_t>> split;  // the (kernel, block)s to split
    for (size_t i = 0; i < probe.plan.size(); i++) {
      const std::string& name = probe.chunks[i].name;
      RegVerdict v;
      if (!reg_verdict(probe, program_of(probe, name), probe.plan[i].waves, &v))
        throw std::runtime_error("kvjit: no kernel descriptor for probe " + name);
      if (v.probe_splits()) split.insert(at[i]);
    }
    if (split.empty()) return;
    for (size_t k = 0; k < img->plan.size(); k++) {
      std::vector<uint32_t> nb;
      for (size_t b = 0; b < img->plan[k].blocks.size(); b++) {
        const uint32_t c = img->plan[k].blocks[b];
        if (split.count({k, b})) nb.insert(nb.end(), {c / 2, c - c / 2});
        else nb.push_back(c);
      }
      img->plan[k].blocks = nb;
    }
  }
}

// key of the plan cache: a hash of the first generated image
std::string jit_plan_key(const JitImage& img) {
  uint64_t h = common_hash(img.common);
  for (size_t i = 0; i < img.kernel_src.size(); i++) h = fnv1a64(img.kernel_src[i], fnv1a64(img.kernel_name[i], h));
  char key[40];
  snprintf(key, sizeof key, "%016llx", (unsigned long long)h);
  return key;
}

}  // namespace

uint64_t code_bytes(const JitImage& img) {
  uint64_t n = 0;
  for (auto& c : img.codes) n += c.size();
  return n;
}

bool jit_load_plan(const std::string& key, JitImage* img) {
  const std::string dir = cache_dir();
  std::vector<char> text;
  if (dir.empty() || !read_file(dir + "/plan-" + key + ".txt", &text)) return false;
  std::vector<JitKernelPlan> plan;
  std::istringstream in(std::string(text.begin(), text.end()));
  for (std::string line; std::getline(in, line);) {
    if (line.rfind("kernel ", 0) != 0) continue;  // kernel <first> <count> <waves> <grouped> <colloops> <block sizes...>
    std::istringstream ls(line.substr(7));
    JitKernelPlan kp{0, 0, 0, {}};
    ls >> kp.first >> kp.count >> kp.waves >> kp.grouped >> kp.colloops;
    uint32_t sum = 0;
    for (uint32_t b; ls >> b; sum += b) kp.blocks.push_back(b);
    if (sum != kp.count || kp.blocks.empty()) return false;
    plan.push_back(kp);
  }
  if (plan.empty()) return false;
  img->plan = plan;
  return true;
}

void jit_save_plan(const std::string& key, const JitImage& img) {
  const std::string dir = cache_dir();
  if (dir.empty()) return;
  std::string t;
  for (const JitKernelPlan& kp : img.plan) {
    t += "kernel " + std::to_string(kp.first) + " " + std::to_string(kp.count) + " " + std::to_string(kp.waves) + " " +
         (kp.grouped ? "1" : "0") + " " + (kp.colloops ? "1" : "0");
    for (uint32_t b : kp.blocks) t += " " + std::to_string(b);
    t += "\n";
  }
  // the code objects of the final kernels (tools/jit_warm.sh keeps these, drops the
  // intermediate probes and re-plans)
  const uint64_t hc = common_hash(img.common);
  for (size_t i = 0; i < img.kernel_src.size(); i++) t += "co " + cache_file(img, i, hc) + "\n";
  for (const JitImage::Variant& v : img.variants) {  // (the output-mode variants' code objects)
    const uint64_t hv = common_hash(variant_common(img, v.full));
    for (size_t i = 0; i < img.kernel_src.size(); i++)
      if (i < v.codes.size() && !v.codes[i].empty()) t += "co " + cache_file(img, i, hv) + "\n";
  }
  write_file_atomic(dir, dir + "/plan-" + key + ".txt", t);
}

// The layout of every kernel's hoist regions, over the settled plan: all of them in three parts
// (JitKernelPlan::grouped) and every per-rule array loop over path columns (JitKernelPlan::
// colloops: a hoist region more per loop), compiled once; a kernel that no longer meets its
// register rules that way (the loads grouped at the top of a region are in flight together)
// steps down, instead of giving up blocks or waves: three parts with its loops walking the node
// rows, then first-use order with column loops, then first-use order with the walk, in which
// it settled.
static void jit_group_regions(const PolicySet& ps, uint32_t chunk, JitImage* img) {
  static const bool kSteps[4][2] = {{true, true}, {true, false}, {false, true}, {false, false}};  // (grouped, colloops)
  std::vector<int> step(img->plan.size(), 0);
  for (int round = 0; round < 4; round++) {
    for (size_t k = 0; k < img->plan.size(); k++) {
      img->plan[k].grouped = kSteps[step[k]][0];
      img->plan[k].colloops = kSteps[step[k]][1];
    }
    jit_generate(ps, chunk, img);
    jit_compile(img);  // (the kernels that did not change: from the cache)
    bool back = false;
    for (size_t k = 0; k < img->plan.size(); k++) {
      RegVerdict v;
      if (!reg_verdict(*img, program_of(*img, img->chunks[k].name), img->plan[k].waves, &v))
        throw std::runtime_error("kvjit: no kernel descriptor for " + img->chunks[k].name);
      if (!v.ships() && step[k] < 3) {
        step[k]++;
        back = true;
      }
    }
    if (!back) return;
  }
}

void jit_build(const PolicySet& ps, JitImage* img) {
  const uint32_t chunk = jit_chunk_rules();
  const char* dump = getenv("KVGPU_JIT_DUMP");
  jit_generate(ps, chunk, img);
  if (dump) write_file(dump, img->source);
  if (!getenv("KVGPU_JIT_SKIP_COMPILE")) {  // (dump-only analysis runs skip it)
    const std::string pkey = jit_plan_key(*img);
    // (a stored plan is final, and if the ladder below still has to change it, a kernel's three-part
    // layout is the first thing to go; a new one is made in first-use order, then given its layouts)
    const bool stored = jit_load_plan(pkey, img);
    if (!stored) {
      for (JitKernelPlan& kp : img->plan) kp.grouped = kp.colloops = false;
      jit_refine_blocks(ps, chunk, img);  // block sizes from probe compiles
    }
    jit_generate(ps, chunk, img);
    // register budget: re-plan kernels that spill until the compiled plan is the final one
    // (the codes must belong to the last generated image: a plan still changing when the
    // rounds run out is an error, never shipped nor cached)
    bool settled = false;
    for (int round = 0; round < 64 && !settled; round++) {
      jit_compile(img);
      settled = !jit_plan_spills(img);
      if (!settled) jit_generate(ps, chunk, img);
    }
    if (!settled)
      throw std::runtime_error("kvjit: the register plan did not settle (kernels still spill after 64 re-plans)");
    if (!stored) jit_group_regions(ps, chunk, img);
    jit_compile_variants(img);  // (output-mode variants of the final kernels)
    jit_save_plan(pkey, *img);
    if (dump) write_file(dump, img->source);  // (the source of the final plan)
  }
  if (const char* co = getenv("KVGPU_JIT_DUMP_CO")) {  // gfx950 code objects (llvm-objdump / readelf)
    for (size_t i = 0; i < img->codes.size(); i++) write_file(std::string(co) + "." + img->kernel_name[i] + ".co", img->codes[i]);
    for (const JitImage::Variant& v : img->variants)  // (output-mode variants: <name>.m<full>)
      for (size_t i = 0; i < v.codes.size(); i++)
        if (!v.codes[i].empty())
          write_file(std::string(co) + "." + img->kernel_name[i] + ".m" + std::to_string(v.full) + ".co", v.codes[i]);
  }
}

}  // namespace kvh
