// jit_sched.cpp -- post-passes over the generated text: the list scheduler of a run's VALU
// code and the resolution of long jumps (jit_int.h).
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "jit_int.h"

namespace wb {
namespace jit {

// ---------------------------------------------------------------- scheduling
// One wave per SIMD (64K instances fill the chip) hides no latency: a VALU instruction
// that needs the result of the one before waits for it (measured: ~12 cycles per
// instruction along a dependent chain against 4 for independent ones). The run's code is
// therefore list-scheduled between barriers (anything but a VALU instruction: scalar
// code, branches, memory, waits), on the registers each instruction names: true, anti
// and output dependences kept, independent chains (BLAKE3's four column / diagonal G
// functions) interleaved.
namespace {
struct SIns {
  std::string text;
  std::vector<int> defs, uses;
  bool wait = false;   // a counted vmcnt wait: defs = the registers of the loads it retires
  int est = 0;         // (wait) estimated cycle its loads are in
  bool store = false;  // a global store: uses its address and data registers
};
}  // namespace

static void regs_of(const std::string &tok, std::vector<int> *out) {
  // vN, v[N:M], sN, s[N:M], vcc (VGPR k -> k, SGPR k -> 1000 + k, vcc -> 2000)
  size_t i = 0;
  while (i < tok.size()) {
    const char ch = tok[i];
    const bool word_start = i == 0 || !(isalnum((unsigned char)tok[i - 1]) || tok[i - 1] == '_');
    if (word_start && tok.compare(i, 3, "vcc") == 0) { out->push_back(2000); i += 3; continue; }
    if (word_start && (ch == 'v' || ch == 's') && i + 1 < tok.size()) {
      const int base = ch == 'v' ? 0 : 1000;
      if (tok[i + 1] == '[') {
        int lo = 0, hi = 0;
        if (sscanf(tok.c_str() + i + 2, "%d:%d", &lo, &hi) == 2)
          for (int r = lo; r <= hi; r++) out->push_back(base + r);
        i = tok.find(']', i) + 1;
        continue;
      }
      if (isdigit((unsigned char)tok[i + 1])) {
        out->push_back(base + atoi(tok.c_str() + i + 1));
        i++;
        while (i < tok.size() && isdigit((unsigned char)tok[i])) i++;
        continue;
      }
    }
    i++;
  }
}

static bool parse_valu(const std::string &line, SIns *ins) {
  ins->text = line;
  if (line.compare(0, 2, "v_") != 0) return false;
  const size_t sp = line.find(' ');
  if (sp == std::string::npos) return false;
  const std::string mn = line.substr(0, sp);
  std::vector<std::string> ops;
  for (size_t at = sp + 1; at <= line.size();) {
    size_t cm = line.find(", ", at);
    if (cm == std::string::npos) cm = line.size();
    ops.push_back(line.substr(at, cm - at));
    at = cm + 2;
  }
  const size_t ndef = mn.find("_co_") != std::string::npos ? 2 : 1;   // v_add_co: vdst, sdst
  for (size_t k = 0; k < ops.size(); k++) regs_of(ops[k], k < ndef ? &ins->defs : &ins->uses);
  return true;
}

std::string schedule(const std::string &body, const JitKnobs &kn) {
  std::vector<std::string> lines;
  for (size_t at = 0; at < body.size();) {
    const size_t nl = body.find('\n', at);
    lines.push_back(body.substr(at, nl - at));
    at = nl + 1;
  }
  std::string out;
  std::vector<SIns> seg;
  auto flush = [&]() {
    const size_t n = seg.size();
    if (n > 1) {
      // dependences: j -> i (j earlier) with a latency in cycles
      constexpr int kIssue = 4, kLat = 12;
      std::vector<std::vector<std::pair<int, int>>> pred(n), succ(n);
      std::map<int, int> last_def;
      std::map<int, std::vector<int>> readers;
      int last_wait = -1;
      for (size_t i = 0; i < n; i++) {
        std::map<int, int> dep;   // pred -> latency
        for (int r : seg[i].uses) {
          auto it = last_def.find(r);
          if (it != last_def.end())
            dep[it->second] = std::max(dep[it->second], seg[size_t(it->second)].wait ? 0 : kLat);
        }
        // waits and stores keep their order (the counts are issue-order counts)
        if ((seg[i].wait || seg[i].store) && last_wait >= 0) dep[last_wait] = std::max(dep[last_wait], 0);
        if (seg[i].wait || seg[i].store) last_wait = int(i);
        for (int r : seg[i].defs) {
          auto it = last_def.find(r);
          if (it != last_def.end()) dep[it->second] = std::max(dep[it->second], 1);
          for (int j : readers[r])
            if (j != int(i)) dep[j] = std::max(dep[j], 1);
        }
        for (auto &d : dep) {
          pred[i].push_back({d.first, d.second});
          succ[size_t(d.first)].push_back({int(i), d.second});
        }
        for (int r : seg[i].uses) readers[r].push_back(int(i));
        for (int r : seg[i].defs) { last_def[r] = int(i); readers[r].clear(); }
      }
      std::vector<int> height(n, 0);   // longest latency path to the segment's end
      for (size_t i = n; i-- > 0;)
        for (auto &s : succ[i]) height[i] = std::max(height[i], height[size_t(s.first)] + s.second);
      std::vector<int> npred(n), at(n, 0);
      for (size_t i = 0; i < n; i++) {
        npred[i] = int(pred[i].size());
        if (seg[i].wait) at[i] = seg[i].est;
      }
      std::vector<int> ready;
      for (size_t i = 0; i < n; i++)
        if (!npred[i]) ready.push_back(int(i));
      int clock = 0;
      while (!ready.empty()) {
        size_t best = 0;
        for (size_t k = 1; k < ready.size(); k++) {
          const int a = ready[k], b = ready[best];
          const int ta = std::max(at[size_t(a)], clock), tb = std::max(at[size_t(b)], clock);
          if (ta < tb || (ta == tb && (height[size_t(a)] > height[size_t(b)] ||
                                       (height[size_t(a)] == height[size_t(b)] && a < b))))
            best = k;
        }
        const int i = ready[best];
        ready.erase(ready.begin() + long(best));
        const int t = std::max(at[size_t(i)], clock);
        clock = seg[size_t(i)].wait ? t : t + kIssue;
        out += seg[size_t(i)].text;
        out += '\n';
        for (auto &s : succ[size_t(i)]) {
          at[size_t(s.first)] = std::max(at[size_t(s.first)], t + s.second);
          if (--npred[size_t(s.first)] == 0) ready.push_back(s.first);
        }
      }
    } else if (n == 1) {
      out += seg[0].text;
      out += '\n';
    }
    seg.clear();
  };
  // Counted waits float: the vector-memory operations issued so far (oldest first, the
  // registers each load writes) tell which loads an "s_waitcnt vmcnt(N)" retires; the
  // wait becomes an instruction of the segment that defines those registers, so their
  // readers stay behind it and independent VALU work moves above it. A label whose
  // arrivals may differ (anything but an inlined call's Lpa / a NaN fix's Lnr return)
  // makes the state unknown until the next full wait, and waits then stay barriers.
  constexpr int kLoadLat = 100, kLoadStep = 22;   // cycles: first L2-hit load, each further
  const bool float_stores = kn.sched_stores;   // (off: stores stay barriers, A/B aid)
  std::vector<std::vector<int>> vq;   // operations in flight, oldest first
  bool known = true;
  int retired = 0;                    // loads retired by this segment's waits so far
  for (const auto &ln : lines) {
    SIns ins;
    if (parse_valu(ln, &ins)) {
      seg.push_back(std::move(ins));
      continue;
    }
    int nwait = -1;
    if (ln.compare(0, 16, "s_waitcnt vmcnt(") == 0 && ln.find("lgkmcnt") == std::string::npos)
      nwait = atoi(ln.c_str() + 16);
    if (nwait >= 0 && known) {
      SIns w;
      w.text = ln;
      w.wait = true;
      while (vq.size() > size_t(nwait)) {
        for (int r : vq.front()) w.defs.push_back(r);
        vq.erase(vq.begin());
        retired++;
      }
      w.est = kLoadLat + kLoadStep * retired;
      seg.push_back(std::move(w));
      continue;
    }
    if (ln.compare(0, 12, "global_store") == 0 && known && float_stores) {
      // a store only reads registers: VALU work moves across it (its data and address
      // registers' writers stay before it, later writers after it)
      SIns st;
      st.text = ln;
      st.store = true;
      const size_t sp = ln.find(' ');
      if (sp != std::string::npos) regs_of(ln.substr(sp + 1), &st.uses);
      seg.push_back(std::move(st));
      vq.push_back({});
      continue;
    }
    flush();
    retired = 0;
    out += ln;
    out += '\n';
    if (ln.compare(0, 11, "global_load") == 0) {
      std::vector<int> d;
      const size_t sp = ln.find(' '), cm = ln.find(',');
      if (sp != std::string::npos && cm != std::string::npos) regs_of(ln.substr(sp + 1, cm - sp - 1), &d);
      vq.push_back(d);
    } else if (ln.compare(0, 7, "global_") == 0 || ln.compare(0, 7, "buffer_") == 0) {
      vq.push_back({});
    } else if (ln.find("vmcnt(0)") != std::string::npos) {
      vq.clear();
      known = true;
    } else if (!ln.empty() && ln.back() == ':' && ln.compare(0, 3, "Lpa") != 0 &&
               ln.compare(0, 3, "Lnr") != 0) {
      known = false;
    }
  }
  flush();
  return out;
}

// long_jump's and cond_jump's placeholders (LJMP / LJCC, jit.cpp) become s_branch /
// s_cbranch_scc1 when the target is surely within its +-128 KiB, else a pc-relative
// s_setpc through s[68:69]
std::string resolve_jumps(const std::string &body) {
  std::vector<std::string> lines;
  for (size_t at = 0; at < body.size();) {
    size_t nl = body.find('\n', at);
    if (nl == std::string::npos) nl = body.size();
    lines.push_back(body.substr(at, nl - at));
    at = nl + 1;
  }
  // an upper bound on the bytes before each line: 12 per instruction (8 + a literal),
  // 64 per alignment
  std::vector<uint64_t> pos(lines.size() + 1, 0);
  std::map<std::string, size_t> lab;
  for (size_t i = 0; i < lines.size(); i++) {
    const std::string &ln = lines[i];
    uint64_t b = 12;
    if (ln.empty() || ln[0] == '.') b = ln.compare(0, 8, ".p2align") == 0 ? 64 : 0;
    if (ln.compare(0, 5, "LJMP ") == 0 || ln.compare(0, 5, "LJCC ") == 0) b = 48;   // (the long form)
    if (!ln.empty() && ln.back() == ':') { lab[ln.substr(0, ln.size() - 1)] = i; b = 0; }
    pos[i + 1] = pos[i] + b;
  }
  std::string out;
  out.reserve(body.size() + body.size() / 4);
  for (size_t i = 0; i < lines.size(); i++) {
    const std::string &ln = lines[i];
    const bool cc = ln.compare(0, 5, "LJCC ") == 0;
    if (ln.compare(0, 5, "LJMP ") != 0 && !cc) { out += ln; out += '\n'; continue; }
    const size_t sp = ln.find(' ', 5);
    const std::string to = ln.substr(5, sp - 5), tag = ln.substr(sp + 1);
    auto it = lab.find(to);
    const uint64_t d = it == lab.end() ? ~0ull
                                       : (pos[it->second] > pos[i] ? pos[it->second] - pos[i]
                                                                    : pos[i] - pos[it->second]);
    if (d < 100000) {
      out += (cc ? "s_cbranch_scc1 " : "s_branch ") + to + "\n";
    } else if (cc) {
      out += "s_cbranch_scc0 " + tag + "_n\n";
      out += "s_getpc_b64 s[68:69]\n" + tag + ":\n";
      out += "s_add_u32 s68, s68, " + to + " - " + tag + "\n";
      out += "s_addc_u32 s69, s69, (" + to + " - " + tag + ") >> 32\n";
      out += "s_setpc_b64 s[68:69]\n" + tag + "_n:\n";
    } else {
      out += "s_getpc_b64 s[68:69]\n" + tag + ":\n";
      out += "s_add_u32 s68, s68, " + to + " - " + tag + "\n";
      out += "s_addc_u32 s69, s69, (" + to + " - " + tag + ") >> 32\n";
      out += "s_setpc_b64 s[68:69]\n";
    }
  }
  return out;
}

}  // namespace jit
}  // namespace wb
