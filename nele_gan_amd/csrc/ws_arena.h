// How a call carves its workspace and how the carve is described to the caller, once for every unit that does either (host only):
// the 256-byte rounding and the bump; WsArena, which bumps fields into the pointer members of a kernel argument struct (EstoiWs, SiibWs,
// HaspiWs, QualWs, EighWs: passed to kernels by value, left as they are) and records each field's offset, unpadded size and element size
// on the host; ws_sections, which writes the {offset, stride, bytes} triples of a *_sections function from those records.
#pragma once
#include <cstdlib>
#include "common.h"

static inline size_t ws_round256(size_t v) { return (v + 255) & ~(size_t)255; }

// `bytes` at *off (the place is returned), the next take 256-byte aligned behind it
static inline size_t ws_bump(size_t* off, size_t bytes) { const size_t at = *off; *off += ws_round256(bytes); return at; }

struct WsField { const void* slot; size_t off, bytes, elem; };   // slot: the pointer member that received the field (its key)

struct WsArena {
    static constexpr int MAXF = 48;                               // the longest carve (HASPI with its quality part) has 40 fields
    char* base;                                                   // nullptr: sizes and fields only, the pointers are set to nullptr
    size_t off = 0;                                               // bytes taken so far: the workspace size once the layout is done
    WsField f[MAXF];
    int n = 0;
    explicit WsArena(void* b) : base(static_cast<char*>(b)) {}

    template <class T>
    void take(T*& p, size_t count) {
        if (n == MAXF) abort();
        const size_t at = ws_bump(&off, sizeof(T) * count);
        f[n++] = WsField{&p, at, sizeof(T) * count, sizeof(T)};
        p = base ? reinterpret_cast<T*>(base + at) : nullptr;
    }
    // the record of the take that filled pointer member `p` (pass the member itself, e.g. at(w.xr))
    template <class T>
    const WsField& at(T* const& p) const {
        for (int i = 0; i < n; ++i)
            if (f[i].slot == &p) return f[i];
        abort();
    }
};

// The section list of a workspace: out[3 k .. 3 k + 2] = {offset, stride, bytes}; utterance b's part of a section is the first `bytes`
// bytes at offset + b * stride, stride 0 = a table all utterances share.  Sections are named by the pointer members the arena filled, in
// the order of the list.  out == nullptr: the sections are counted only.
struct WsSections {
    const WsArena& a;
    int B;
    long long* out;
    int k = 0;
    void put(size_t off, size_t stride, size_t bytes) {
        if (out) { out[3 * k] = (long long)off; out[3 * k + 1] = (long long)stride; out[3 * k + 2] = (long long)bytes; }
        ++k;
    }
    void row(const WsField& fd, size_t of) { put(fd.off, fd.bytes / (size_t)B, fd.bytes / (size_t)B / of); }
    template <class... T> void rows(T* const&... p) { (row(a.at(p), 1), ...); }          // per-utterance fields [B][...]: whole rows
    template <class... T> void half_rows(T* const&... p) { (row(a.at(p), 2), ...); }     // fields [B][2][...]: the first (clean-signal) half of each row
    template <class... T> void shared(T* const&... p) { (put(a.at(p).off, 0, a.at(p).bytes), ...); }   // tables all utterances share
    template <class T> void shared_entry0(T* const& p, size_t entries) { put(a.at(p).off, 0, a.at(p).bytes / entries); }   // the first of `entries` equal parts
    // one element per utterance of field `fd` of the workspace nested in field `outer`
    template <class T> void nested_elems(T* const& outer, const WsField& fd) { put(a.at(outer).off + fd.off, fd.elem, fd.elem); }
};

// The body of a *_sections function: `list(WsSections&)` names the sections of arena `a`; it runs once to count them - the minimum
// `max_sections` is the length of the list itself - and once more to write them.  Returns the number of sections or a negative status.
template <class List>
static int ws_sections(const char* who, const WsArena& a, int B, long long* out, int max_sections, List list) {
    WsSections dry{a, B, nullptr};
    list(dry);
    NELE_CHECK_ARG(max_sections >= dry.k, "%s: bad arguments (%d sections)", who, dry.k);
    WsSections s{a, B, out};
    list(s);
    return s.k;
}
