// nem_gff.hip -- see nem_gff.hpp.  The kernels, then the C entry points (nemgpu_gff_*).
#include <hip/hip_runtime.h>

#include <climits>
#include <memory>
#include <string>
#include <vector>

#include "nem_gff.hpp"
#include "nem_internal.hpp"
#include "nem_scan.hpp"
#include "nem_table.hpp"

namespace nemk {
namespace {

using seg::kThreads;

__device__ inline bool is_ws(unsigned char c) { return c == 32 || (c >= 9 && c <= 13) || (c >= 28 && c <= 31); }   // str.isspace() below 0x80

// [a, b) without the whitespace at either end; an all-whitespace run is the empty span at b
__device__ inline void strip(const char* __restrict__ t, int& a, int& b)
{
    while (a < b && is_ws((unsigned char)t[a])) a++;
    while (b > a && is_ws((unsigned char)t[b - 1])) b--;
}

// ---- marks: the bytes at which a line / a token starts ------------------------------------------------------------
struct LineStart { __device__ bool operator()(unsigned char prev, unsigned char cur) const { return prev == '\n' || (prev == '\r' && cur != '\n'); } };
struct TokenStart { __device__ bool operator()(unsigned char prev, unsigned char cur) const { return !is_ws(cur) && is_ws(prev); } };

// the marks among the 16 bytes from `base` as a bit mask; byte 0 of the text counts as preceded by '\n'
template <class Mark> __device__ inline uint32_t marks16(const char* __restrict__ t, long long n, long long base, Mark mark)
{
    unsigned char c[kGffBytes];
    if (base + kGffBytes <= n) {
        const uint4 v = *reinterpret_cast<const uint4*>(t + base);        // (the text's buffer is 256-byte aligned, base a multiple of 16)
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < kGffBytes; j++) c[j] = (unsigned char)(w[j >> 2] >> (8 * (j & 3)));
    } else {
#pragma unroll
        for (int j = 0; j < kGffBytes; j++) c[j] = base + j < n ? (unsigned char)t[base + j] : (unsigned char)0;
    }
    unsigned char prev = base > 0 ? (unsigned char)t[base - 1] : (unsigned char)'\n';
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < kGffBytes; j++) {
        if (base + j < n && mark(prev, c[j])) m |= 1u << j;
        prev = c[j];
    }
    return m;
}

template <class Mark> __global__ __launch_bounds__(kGffThreads) void k_mark_count(const char* __restrict__ t, long long n, Mark mark, int* __restrict__ count)
{
    const long long i = (long long)blockIdx.x * kGffThreads + threadIdx.x;
    if (i * kGffBytes < n) count[i] = __popc(marks16(t, n, i * kGffBytes, mark));
}

// at[before[i] + j] = the j-th mark of thread i's bytes (before: the exclusive scan of the counts)
template <class Mark>
__global__ __launch_bounds__(kGffThreads) void k_mark_emit(const char* __restrict__ t, long long n, Mark mark, const int* __restrict__ before, int total,
                                                           int* __restrict__ at)
{
    const long long i = (long long)blockIdx.x * kGffThreads + threadIdx.x;
    if (i * kGffBytes >= n) return;
    uint32_t m = marks16(t, n, i * kGffBytes, mark);
    int p = before[i];
    while (m && p < total) {
        const int j = __ffs(m) - 1;
        at[p++] = (int)(i * kGffBytes + j);
        m &= m - 1;
    }
}

// ---- tables keyed by bytes ------------------------------------------------------------------------------------------
__device__ inline uint64_t hash_bytes(const char* __restrict__ t, int len, uint32_t salt, uint64_t keep)
{
    uint64_t h = 0xcbf29ce484222325ull ^ ((uint64_t)salt * 0x9E3779B97F4A7C15ull);
    for (int j = 0; j < len; j++) { h ^= (unsigned char)t[j]; h *= 0x100000001b3ull; }
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33;
    return h & keep;
}

__device__ inline bool same_bytes(const char* __restrict__ a, const char* __restrict__ b, int len)
{
    for (int j = 0; j < len; j++) if (a[j] != b[j]) return false;
    return true;
}

// the keys of a table: item i is the bytes [off[at], off[at] + len[at]) of text with at = map ? map[i] : i, and salt[at]
struct Keys {
    const char* text;
    const int* off;
    const int* len;
    const int* salt;      // may be null: 0
    const int* map;       // may be null: the identity
    __device__ int at(int i) const { return map ? map[i] : i; }
};

// item i enters the table: its class's slot afterwards holds the least (kMax: the greatest) item of the class.
// slot_of[i] = that slot.  The table has at least twice as many slots as items, so a probe ends.
template <bool kMax>
__global__ __launch_bounds__(kThreads) void k_insert(Keys k, int count, const int* __restrict__ sel, int want, int* __restrict__ tbl, uint32_t mask, uint64_t keep,
                                                     int* __restrict__ slot_of)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    if (sel && sel[i] != want) { if (slot_of) slot_of[i] = -1; return; }
    const int me = k.at(i);
    const int len = k.len[me], salt = k.salt ? k.salt[me] : 0;
    const char* mine = k.text + k.off[me];
    uint32_t slot = (uint32_t)hash_bytes(mine, len, (uint32_t)salt, keep) & mask;
    int found = -1;
    for (uint32_t probe = 0; probe <= mask; probe++, slot = (slot + 1) & mask) {
        const int cur = atomicCAS(&tbl[slot], -1, i);
        if (cur == -1 || cur == i) { found = (int)slot; break; }
        const int other = k.at(cur);
        if (k.len[other] == len && (k.salt ? k.salt[other] : 0) == salt && same_bytes(k.text + k.off[other], mine, len)) {
            if (kMax) atomicMax(&tbl[slot], i); else atomicMin(&tbl[slot], i);
            found = (int)slot;
            break;
        }
    }
    if (slot_of) slot_of[i] = found;
}

// the item of the class of the bytes q[0, qlen) (salt 0) in a finished table, -1 if it has none
__device__ inline int table_find(const int* __restrict__ tbl, uint32_t mask, uint64_t keep, const char* __restrict__ text, const int* __restrict__ off,
                                 const int* __restrict__ len, const char* __restrict__ q, int qlen)
{
    uint32_t slot = (uint32_t)hash_bytes(q, qlen, 0u, keep) & mask;
    for (uint32_t probe = 0; probe <= mask; probe++, slot = (slot + 1) & mask) {
        const int cur = tbl[slot];
        if (cur < 0) return -1;
        if (len[cur] == qlen && same_bytes(text + off[cur], q, qlen)) return cur;
    }
    return -1;
}

// ---- the families table ----------------------------------------------------------------------------------------------
// a token's length, and whether it is the first of its line (the family): first[i] = i or -1
__global__ __launch_bounds__(kThreads) void k_tokens(const char* __restrict__ t, int n, const int* __restrict__ off, int nt, int* __restrict__ len,
                                                     int* __restrict__ first, int* __restrict__ is_first)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= nt) return;
    const int a = off[i];
    int b = a;
    while (b < n && !is_ws((unsigned char)t[b])) b++;
    len[i] = b - a;
    int p = a - 1;
    bool head = true;                                      // (no token between the line's start and this one)
    while (p >= 0) {
        const unsigned char c = (unsigned char)t[p];
        if (c == '\n' || c == '\r') break;
        if (!is_ws(c)) { head = false; break; }
        p--;
    }
    first[i] = head ? i : -1;
    is_first[i] = head ? 1 : 0;
}

// a family token that is its name's least one is a distinct family
__global__ __launch_bounds__(kThreads) void k_class_heads(const int* __restrict__ tbl, const int* __restrict__ slot_of, int count, int* __restrict__ head)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < count) head[i] = slot_of[i] >= 0 && tbl[slot_of[i]] == i ? 1 : 0;
}

// tok_tf[i] = the distinct family of token i's line; the distinct families' spans
__global__ __launch_bounds__(kThreads) void k_token_family(const int* __restrict__ tbl, const int* __restrict__ slot_of, const int* __restrict__ line_first,
                                                           const int* __restrict__ head, const int* __restrict__ before, const int* __restrict__ off,
                                                           const int* __restrict__ len, int nt, int* __restrict__ tok_tf, int* __restrict__ spans)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= nt) return;
    const int f = line_first[i];                           // (>= 0: a line's first token precedes its others)
    const int s = f >= 0 ? slot_of[f] : -1;
    tok_tf[i] = s >= 0 ? before[tbl[s]] : -1;
    if (head[i]) { spans[2 * before[i]] = off[i]; spans[2 * before[i] + 1] = len[i]; }
}

// ---- a batch ---------------------------------------------------------------------------------------------------------
struct Batch {
    const char* text;
    int n, nf, nl;
    const int* fs;            // [nf] a file's first byte
    const int* fe;            // [nf] past its last
    const int* line_off;      // [nl]
};

// line l: its file, and [a, b) without the terminator; false: the line is none (it starts at or after its file's end)
__device__ inline bool line_bounds(const Batch& B, int l, int& f, int& a, int& b)
{
    a = B.line_off[l];
    f = seg::last_le(B.fs, B.nf, a);
    const int fe = B.fe[f];
    if (a >= fe) return false;
    b = l + 1 < B.nl ? B.line_off[l + 1] : B.n;
    if (b > fe) b = fe;
    if (b > a && B.text[b - 1] == '\n') { b--; if (b > a && B.text[b - 1] == '\r') b--; }
    else if (b > a && B.text[b - 1] == '\r') b--;
    return true;
}

__device__ inline bool is_pragma(const char* __restrict__ t, int a, int b) { return b - a >= 2 && t[a] == '#' && t[a + 1] == '#'; }

__global__ __launch_bounds__(kThreads) void k_file_lines(Batch B, int* __restrict__ first_line, int* __restrict__ fasta_line)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= B.nf) return;
    first_line[f] = seg::lower_bound(B.line_off, 0, B.nl, B.fs[f]);
    fasta_line[f] = INT_MAX;
}

__global__ __launch_bounds__(kThreads) void k_fasta(Batch B, int* __restrict__ fasta_line)
{
    const int l = blockIdx.x * kThreads + threadIdx.x;
    if (l >= B.nl) return;
    int f, a, b;
    if (!line_bounds(B, l, f, a, b) || !is_pragma(B.text, a, b) || b - a < 7) return;
    const char* t = B.text + a + 2;
    if (t[0] == 'F' && t[1] == 'A' && t[2] == 'S' && t[3] == 'T' && t[4] == 'A') atomicMin(&fasta_line[f], l);
}

__device__ inline void refuse(unsigned long long* error, int f, int line, int code)
{
    atomicMin(error, ((unsigned long long)f << 40) | ((unsigned long long)(uint32_t)line << 8) | (unsigned long long)code);
}

// an optional sign and ASCII digits within int32
__device__ inline bool parse_int32(const char* __restrict__ t, int a, int b, int* out)
{
    bool neg = false;
    if (a < b && (t[a] == '+' || t[a] == '-')) { neg = t[a] == '-'; a++; }
    if (a >= b) return false;
    long long v = 0;
    for (; a < b; a++) {
        const int dgt = t[a] - '0';
        if (dgt < 0 || dgt > 9) return false;
        v = v * 10 + dgt;
        if (v > (1ll << 32)) v = 1ll << 32;                // (out of range for good; the rest must still be digits)
    }
    if (neg) v = -v;
    if (v < -(1ll << 31) || v >= (1ll << 31)) return false;
    *out = (int)v;
    return true;
}

__device__ inline bool key_is(const char* __restrict__ t, int a, int b, const char* word, int n)
{
    if (b - a != n) return false;
    for (int j = 0; j < n; j++) {
        char c = t[a + j];
        if (c >= 'a' && c <= 'z') c -= 32;
        if (c != word[j]) return false;
    }
    return true;
}

struct FamTable {
    const char* text;
    const int* tok_off;
    const int* tok_len;
    const int* tok_tf;
    const int* tbl;
    uint32_t mask;
    uint64_t keep;
};

// the records of the lines, by line: is_cds, file, start, end, fam and the five spans
struct Records {
    int* is_cds;
    int* file;
    int* start;
    int* end;
    int* fam;
    int* span_off;            // [kGffSpans][nl]
    int* span_len;
};

__global__ __launch_bounds__(kThreads) void k_parse(Batch B, FamTable F, int infer, const int* __restrict__ first_line, const int* __restrict__ fasta_line,
                                                    Records R, unsigned long long* __restrict__ error)
{
    const int l = blockIdx.x * kThreads + threadIdx.x;
    if (l >= B.nl) return;
    R.is_cds[l] = 0;
    int f, a, b;
    if (!line_bounds(B, l, f, a, b) || l >= fasta_line[f] || is_pragma(B.text, a, b)) return;
    const char* t = B.text;
    int cut[11];                                           // field j is (cut[j] + 1, cut[j + 1]); at most ten are told apart
    int nfld = 1;
    cut[0] = a - 1;
    for (int p = a; p < b && nfld < 10; p++) if (t[p] == '\t') cut[nfld++] = p;
    cut[nfld] = b;
    const int line = l - first_line[f];
    if (nfld < 3) { refuse(error, f, line, kGffFields3); return; }
    int xa = cut[2] + 1, xb = cut[3];
    strip(t, xa, xb);
    if (!(xb - xa == 3 && t[xa] == 'C' && t[xa + 1] == 'D' && t[xa + 2] == 'S')) return;
    if (nfld < 9) { refuse(error, f, line, kGffFields9); return; }
    // the attributes: split on ';', the empty parts dropped, each stripped and split on its one '='
    int ga = cut[8] + 1, gb = cut[9];
    strip(t, ga, gb);
    int id_a = -1, id_b = -1, nm_a = -1, nm_b = -1, ge_a = -1, ge_b = -1, pr_a = -1, pr_b = -1;
    for (int at = ga; at <= gb;) {
        int stop = at;
        while (stop < gb && t[stop] != ';') stop++;
        if (stop > at) {
            int pa = at, pb = stop;
            strip(t, pa, pb);
            int eq = -1, neq = 0;
            for (int p = pa; p < pb; p++) if (t[p] == '=') { if (eq < 0) eq = p; neq++; }
            if (neq != 1) { refuse(error, f, line, kGffAttr); return; }
            if (key_is(t, pa, eq, "ID", 2)) { id_a = eq + 1; id_b = pb; }
            else if (key_is(t, pa, eq, "NAME", 4)) { nm_a = eq + 1; nm_b = pb; }
            else if (key_is(t, pa, eq, "GENE", 4)) { ge_a = eq + 1; ge_b = pb; }
            else if (key_is(t, pa, eq, "PRODUCT", 7)) { pr_a = eq + 1; pr_b = pb; }
        }
        at = stop + 1;
    }
    if (id_a < 0) { refuse(error, f, line, kGffNoId); return; }
    const int tok = table_find(F.tbl, F.mask, F.keep, F.text, F.tok_off, F.tok_len, t + id_a, id_b - id_a);
    if (tok < 0 && !infer) { refuse(error, f, line, kGffUnknown); return; }
    int sa = cut[3] + 1, sb = cut[4], ea = cut[4] + 1, eb = cut[5], start = 0, end = 0;
    strip(t, sa, sb);
    strip(t, ea, eb);
    if (!parse_int32(t, sa, sb, &start)) { refuse(error, f, line, kGffStart); return; }
    if (!parse_int32(t, ea, eb, &end)) { refuse(error, f, line, kGffEnd); return; }
    if (nm_a < 0) { nm_a = ge_a; nm_b = ge_b; }
    if (nm_a < 0) { nm_a = id_a; nm_b = id_a; }            // (absent: the empty span at the ID)
    if (pr_a < 0) { pr_a = id_a; pr_b = id_a; }
    int da = cut[6] + 1, db = cut[7], ca = cut[0] + 1, cb = cut[1];
    strip(t, da, db);
    strip(t, ca, cb);
    R.is_cds[l] = 1;
    R.file[l] = f; R.start[l] = start; R.end[l] = end;
    R.fam[l] = tok >= 0 ? F.tok_tf[tok] : -1;
    const int so[kGffSpans] = {id_a, nm_a, pr_a, da, ca}, sl[kGffSpans] = {id_b - id_a, nm_b - nm_a, pr_b - pr_a, db - da, cb - ca};
#pragma unroll
    for (int j = 0; j < kGffSpans; j++) { R.span_off[(size_t)j * B.nl + l] = so[j]; R.span_len[(size_t)j * B.nl + l] = sl[j]; }
}

// gene_line[before[l]] = l for the CDS lines (before: the exclusive scan of is_cds)
__global__ __launch_bounds__(kThreads) void k_gene_lines(const int* __restrict__ is_cds, const int* __restrict__ before, int nl, int g, int* __restrict__ gene_line)
{
    const int l = blockIdx.x * kThreads + threadIdx.x;
    if (l < nl && is_cds[l] && before[l] < g) gene_line[before[l]] = l;
}

// a gene that is not the least of its (file, ID) is refused at its own line
__global__ __launch_bounds__(kThreads) void k_duplicates(const int* __restrict__ tbl, const int* __restrict__ slot_of, const int* __restrict__ gene_line,
                                                         const int* __restrict__ file, const int* __restrict__ first_line, int g,
                                                         unsigned long long* __restrict__ error)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= g || slot_of[i] < 0 || tbl[slot_of[i]] == i) return;
    const int l = gene_line[i], f = file[l];
    refuse(error, f, l - first_line[f], kGffDup);
}

// key[i] = (the gene's contig, START with its sign bit flipped), val[i] = i; the contig: its class's head's rank
__global__ __launch_bounds__(kThreads) void k_sort_keys(const int* __restrict__ tbl, const int* __restrict__ slot_of, const int* __restrict__ before,
                                                        const int* __restrict__ gene_line, const int* __restrict__ start, int g, uint64_t* __restrict__ key,
                                                        uint32_t* __restrict__ val)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= g) return;
    const int s = slot_of[i];
    const uint32_t contig = s >= 0 ? (uint32_t)before[tbl[s]] : 0u;
    key[i] = ((uint64_t)contig << 32) | ((uint32_t)start[gene_line[i]] ^ 0x80000000u);
    val[i] = (uint32_t)i;
}

struct Sorted {
    int* file;
    int* start;
    int* end;
    int* fam;
    int* contig;
    int* span_off;            // [kGffSpans][g]
    int* span_len;
};

__global__ __launch_bounds__(kThreads) void k_gather(const uint64_t* __restrict__ key, const uint32_t* __restrict__ val, const int* __restrict__ gene_line,
                                                     Records R, int nl, int g, Sorted S)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= g) return;
    const int l = gene_line[val[p]];
    S.file[p] = R.file[l]; S.start[p] = R.start[l]; S.end[p] = R.end[l]; S.fam[p] = R.fam[l];
    S.contig[p] = (int)(key[p] >> 32);
#pragma unroll
    for (int j = 0; j < kGffSpans; j++) {
        S.span_off[(size_t)j * g + p] = R.span_off[(size_t)j * nl + l];
        S.span_len[(size_t)j * g + p] = R.span_len[(size_t)j * nl + l];
    }
}

// where a file's ##FASTA line starts (its end if it has none)
__global__ __launch_bounds__(kThreads) void k_fasta_off(Batch B, const int* __restrict__ fasta_line, int* __restrict__ fasta_off)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f < B.nf) fasta_off[f] = fasta_line[f] == INT_MAX ? B.fe[f] : B.line_off[fasta_line[f]];
}

// ---- the families' ids and the repeated ones -----------------------------------------------------------------------
// first[name] = the least walk position of a gene of that name
__global__ __launch_bounds__(kThreads) void k_first_gene(const int* __restrict__ name, int g, int* __restrict__ first)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p < g) atomicMin(&first[name[p]], p);
}

__global__ __launch_bounds__(kThreads) void k_first_flags(const int* __restrict__ name, const int* __restrict__ first, int g, int* __restrict__ head)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p < g) head[p] = first[name[p]] == p ? 1 : 0;
}

// a gene's family id: the rank of its name's first gene among the first genes; order[id] = the name; the key of the
// gene's (organism, family) pair
__global__ __launch_bounds__(kThreads) void k_family_ids(const int* __restrict__ name, const int* __restrict__ first, const int* __restrict__ head,
                                                         const int* __restrict__ before, const int* __restrict__ org, int g, int* __restrict__ genes,
                                                         int* __restrict__ order, uint64_t* __restrict__ key)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= g) return;
    const int id = before[first[name[p]]];
    genes[p] = id;
    if (head[p]) order[id] = name[p];
    key[p] = ((uint64_t)(uint32_t)org[p] << 32) | (uint32_t)id;
}

// among the sorted pairs a family occurs more than lim times in an organism where a pair equals the one lim places on
__global__ __launch_bounds__(kThreads) void k_repeated(const uint64_t* __restrict__ key, int g, int lim, uint8_t* __restrict__ repeated)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p < g - lim && key[p] == key[p + lim]) repeated[(uint32_t)key[p]] = 1;
}

uint32_t table_slots(int items) { uint32_t s = 16; while (s < 2u * (uint32_t)std::max(items, 0) + 1u) s <<= 1; return s; }

// at = the marks of text[0, n), *total their number (a wait inside: the count sizes the list)
template <class Mark> hipError_t marks(seg::Scratch& mem, const char* text, long long n, Mark mark, int** at, int* total, hipStream_t s)
{
    *at = nullptr; *total = 0;
    const long long nth = (n + kGffBytes - 1) / kGffBytes;
    if (nth == 0) return mem.alloc(at, 1);
    int *count, *partial, *dtotal;
    HIPTRY(mem.alloc(&count, (size_t)nth));
    HIPTRY(mem.alloc(&partial, (size_t)(nth / seg::kScanTile + 2)));
    HIPTRY(mem.alloc(&dtotal, 1));
    const int nb = (int)((nth + kGffThreads - 1) / kGffThreads);
    hipLaunchKernelGGL((k_mark_count<Mark>), dim3(nb), dim3(kGffThreads), 0, s, text, n, mark, count);
    seg::scan<int, seg::OpSum<int>, false>(count, count, (int)nth, seg::OpSum<int>(), 0, partial, dtotal, s);
    HIPTRY(hipMemcpyAsync(total, dtotal, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPTRY(hipStreamSynchronize(s));
    HIPTRY(mem.alloc(at, (size_t)*total));
    hipLaunchKernelGGL((k_mark_emit<Mark>), dim3(nb), dim3(kGffThreads), 0, s, text, n, mark, (const int*)count, *total, *at);
    return hipGetLastError();
}

// the exclusive sum of flag[0, n) in `before`, its total in *total (a wait inside)
hipError_t ranks(seg::Scratch& mem, const int* flag, int n, int** before, int* total, hipStream_t s)
{
    int *partial, *dtotal;
    HIPTRY(mem.alloc(before, (size_t)n));
    HIPTRY(mem.alloc(&partial, (size_t)(n / seg::kScanTile + 2)));
    HIPTRY(mem.alloc(&dtotal, 1));
    seg::scan<int, seg::OpSum<int>, false>(flag, *before, n, seg::OpSum<int>(), 0, partial, dtotal, s);
    HIPTRY(hipMemcpyAsync(total, dtotal, sizeof(int), hipMemcpyDeviceToHost, s));
    return hipStreamSynchronize(s);
}

hipError_t new_table(seg::Scratch& mem, int items, int** tbl, uint32_t* mask, hipStream_t s)
{
    const uint32_t slots = table_slots(items);
    HIPTRY(mem.alloc(tbl, (size_t)slots));
    *mask = slots - 1;
    return hipMemsetAsync(*tbl, 0xFF, (size_t)slots * sizeof(int), s);
}

}  // namespace
}  // namespace nemk

using namespace nemk;

struct nemgpu_gff {
    int device = 0;
    hipStream_t stream = nullptr;
    uint64_t keep = ~0ull;
    seg::Scratch table;                                    // the families table, for the handle's life
    FamTable fam{};
    int n_families = 0;
    std::vector<int32_t> family_spans;                     // [n_families][2]
    std::unique_ptr<seg::Scratch> batch;                   // the last batch's result, until the next
    Sorted out{};
    int* fasta_off = nullptr;
    int g = 0, contigs = 0, files = 0;
    hipEvent_t ev[kGffStages + 1] = {};
    float stage_ms[kGffStages] = {};
};

namespace {

void gff_free(nemgpu_gff* h)
{
    h->batch.reset();
    for (hipEvent_t e : h->ev) if (e) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

hipError_t build_families(nemgpu_gff* h, const char* host_text, long long n)
{
    seg::Scratch tmp;
    seg::Scratch& keepmem = h->table;
    hipStream_t s = h->stream;
    char* text;
    HIPTRY(keepmem.alloc(&text, a256((size_t)n + 16)));
    if (n) HIPTRY(hipMemcpyAsync(text, host_text, (size_t)n, hipMemcpyHostToDevice, s));
    int *tok_off_tmp, nt = 0;
    HIPTRY(marks(tmp, text, n, TokenStart(), &tok_off_tmp, &nt, s));
    int *tok_off, *tok_len, *tok_tf, *first, *is_first, *line_first, *slot_of, *head, *before, *partial, *tbl_fam, *tbl_gene, *spans;
    uint32_t mask_fam, mask_gene;
    HIPTRY(keepmem.alloc(&tok_off, (size_t)nt));
    HIPTRY(keepmem.alloc(&tok_len, (size_t)nt));
    HIPTRY(keepmem.alloc(&tok_tf, (size_t)nt));
    HIPTRY(new_table(keepmem, nt, &tbl_gene, &mask_gene, s));
    h->fam = FamTable{text, tok_off, tok_len, tok_tf, tbl_gene, mask_gene, h->keep};
    h->n_families = 0;
    if (nt == 0) return hipStreamSynchronize(s);
    HIPTRY(hipMemcpyAsync(tok_off, tok_off_tmp, (size_t)nt * sizeof(int), hipMemcpyDeviceToDevice, s));
    HIPTRY(tmp.alloc(&first, (size_t)nt));
    HIPTRY(tmp.alloc(&is_first, (size_t)nt));
    HIPTRY(tmp.alloc(&line_first, (size_t)nt));
    HIPTRY(tmp.alloc(&slot_of, (size_t)nt));
    HIPTRY(tmp.alloc(&head, (size_t)nt));
    HIPTRY(tmp.alloc(&partial, (size_t)(nt / seg::kScanTile + 2)));
    HIPTRY(new_table(tmp, nt, &tbl_fam, &mask_fam, s));
    const int nb = seg::blocks(nt);
    hipLaunchKernelGGL(k_tokens, dim3(nb), dim3(kThreads), 0, s, (const char*)text, (int)n, (const int*)tok_off, nt, tok_len, first, is_first);
    seg::scan<int, seg::OpMax, true>(first, line_first, nt, seg::OpMax(), -1, partial, (int*)nullptr, s);
    const Keys keys{text, tok_off, tok_len, nullptr, nullptr};
    hipLaunchKernelGGL((k_insert<false>), dim3(nb), dim3(kThreads), 0, s, keys, nt, (const int*)is_first, 1, tbl_fam, mask_fam, h->keep, slot_of);
    hipLaunchKernelGGL(k_class_heads, dim3(nb), dim3(kThreads), 0, s, (const int*)tbl_fam, (const int*)slot_of, nt, head);
    HIPTRY(ranks(tmp, head, nt, &before, &h->n_families, s));
    HIPTRY(tmp.alloc(&spans, (size_t)h->n_families * 2));
    hipLaunchKernelGGL(k_token_family, dim3(nb), dim3(kThreads), 0, s, (const int*)tbl_fam, (const int*)slot_of, (const int*)line_first, (const int*)head,
                       (const int*)before, (const int*)tok_off, (const int*)tok_len, nt, tok_tf, spans);
    hipLaunchKernelGGL((k_insert<true>), dim3(nb), dim3(kThreads), 0, s, keys, nt, (const int*)is_first, 0, tbl_gene, mask_gene, h->keep, (int*)nullptr);
    HIPTRY(hipGetLastError());
    h->family_spans.resize((size_t)h->n_families * 2);
    if (h->n_families) HIPTRY(hipMemcpyAsync(h->family_spans.data(), spans, (size_t)h->n_families * 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    return hipStreamSynchronize(s);
}

hipError_t run_batch(nemgpu_gff* h, const char* host_text, long long n, const int32_t* file_start, const int32_t* file_end, int nf, int infer,
                     unsigned long long* error_out)
{
    h->batch.reset(new seg::Scratch());
    seg::Scratch& mem = *h->batch;
    hipStream_t s = h->stream;
    h->g = h->contigs = 0;
    h->files = nf;
    h->out = Sorted{};
    *error_out = kGffNoError;
    int stage = 0;
    HIPTRY(hipEventRecord(h->ev[stage++], s));
    char* text;
    int *fs, *fe, *first_line, *fasta_line;
    unsigned long long* error;
    HIPTRY(mem.alloc(&text, a256((size_t)n + 16)));
    HIPTRY(mem.alloc(&fs, (size_t)nf));
    HIPTRY(mem.alloc(&fe, (size_t)nf));
    HIPTRY(mem.alloc(&first_line, (size_t)nf));
    HIPTRY(mem.alloc(&fasta_line, (size_t)nf));
    HIPTRY(mem.alloc(&h->fasta_off, (size_t)nf));
    HIPTRY(mem.alloc(&error, 1));
    if (n) HIPTRY(hipMemcpyAsync(text, host_text, (size_t)n, hipMemcpyHostToDevice, s));
    HIPTRY(hipMemcpyAsync(fs, file_start, (size_t)nf * sizeof(int), hipMemcpyHostToDevice, s));
    HIPTRY(hipMemcpyAsync(fe, file_end, (size_t)nf * sizeof(int), hipMemcpyHostToDevice, s));
    HIPTRY(hipMemsetAsync(error, 0xFF, sizeof(unsigned long long), s));
    HIPTRY(hipEventRecord(h->ev[stage++], s));
    // the lines, and where every file's begin and its ##FASTA ends it
    int* line_off;
    int nl = 0;
    HIPTRY(marks(mem, text, n, LineStart(), &line_off, &nl, s));
    const Batch B{text, (int)n, nf, nl, fs, fe, line_off};
    hipLaunchKernelGGL(k_file_lines, dim3(seg::blocks(nf)), dim3(kThreads), 0, s, B, first_line, fasta_line);
    if (nl) hipLaunchKernelGGL(k_fasta, dim3(seg::blocks(nl)), dim3(kThreads), 0, s, B, fasta_line);
    HIPTRY(hipEventRecord(h->ev[stage++], s));
    // the lines' records, the CDS lines' ranks
    Records R{};
    int *before_line = nullptr, g = 0;
    if (nl) {
        HIPTRY(mem.alloc(&R.is_cds, (size_t)nl));
        HIPTRY(mem.alloc(&R.file, (size_t)nl));
        HIPTRY(mem.alloc(&R.start, (size_t)nl));
        HIPTRY(mem.alloc(&R.end, (size_t)nl));
        HIPTRY(mem.alloc(&R.fam, (size_t)nl));
        HIPTRY(mem.alloc(&R.span_off, (size_t)nl * kGffSpans));
        HIPTRY(mem.alloc(&R.span_len, (size_t)nl * kGffSpans));
        hipLaunchKernelGGL(k_parse, dim3(seg::blocks(nl)), dim3(kThreads), 0, s, B, h->fam, infer, (const int*)first_line, (const int*)fasta_line, R, error);
        HIPTRY(ranks(mem, R.is_cds, nl, &before_line, &g, s));
    }
    HIPTRY(hipEventRecord(h->ev[stage++], s));
    int contigs = 0;
    const uint64_t* key_out = nullptr;
    const uint32_t* val_out = nullptr;
    int* gene_line = nullptr;
    if (g) {
        // the contigs by first appearance, the IDs that occur twice in a file
        int *slot_contig, *slot_id, *tbl_contig, *tbl_id, *head, *before;
        uint32_t mask_contig, mask_id;
        HIPTRY(mem.alloc(&gene_line, (size_t)g));
        HIPTRY(mem.alloc(&slot_contig, (size_t)g));
        HIPTRY(mem.alloc(&slot_id, (size_t)g));
        HIPTRY(mem.alloc(&head, (size_t)g));
        HIPTRY(new_table(mem, g, &tbl_contig, &mask_contig, s));
        HIPTRY(new_table(mem, g, &tbl_id, &mask_id, s));
        const int nb = seg::blocks(g);
        hipLaunchKernelGGL(k_gene_lines, dim3(seg::blocks(nl)), dim3(kThreads), 0, s, (const int*)R.is_cds, (const int*)before_line, nl, g, gene_line);
        const Keys contig_keys{text, R.span_off + (size_t)4 * nl, R.span_len + (size_t)4 * nl, R.file, gene_line};
        const Keys id_keys{text, R.span_off, R.span_len, R.file, gene_line};
        hipLaunchKernelGGL((k_insert<false>), dim3(nb), dim3(kThreads), 0, s, contig_keys, g, (const int*)nullptr, 0, tbl_contig, mask_contig, h->keep, slot_contig);
        hipLaunchKernelGGL((k_insert<false>), dim3(nb), dim3(kThreads), 0, s, id_keys, g, (const int*)nullptr, 0, tbl_id, mask_id, h->keep, slot_id);
        hipLaunchKernelGGL(k_duplicates, dim3(nb), dim3(kThreads), 0, s, (const int*)tbl_id, (const int*)slot_id, (const int*)gene_line, (const int*)R.file,
                           (const int*)first_line, g, error);
        hipLaunchKernelGGL(k_class_heads, dim3(nb), dim3(kThreads), 0, s, (const int*)tbl_contig, (const int*)slot_contig, g, head);
        HIPTRY(ranks(mem, head, g, &before, &contigs, s));
        HIPTRY(hipEventRecord(h->ev[stage++], s));
        // one stable sort by (contig, START)
        uint64_t *k0, *k1;
        uint32_t *v0, *v1;
        HIPTRY(mem.alloc(&k0, (size_t)g));
        HIPTRY(mem.alloc(&k1, (size_t)g));
        HIPTRY(mem.alloc(&v0, (size_t)g));
        HIPTRY(mem.alloc(&v1, (size_t)g));
        hipLaunchKernelGGL(k_sort_keys, dim3(nb), dim3(kThreads), 0, s, (const int*)tbl_contig, (const int*)slot_contig, (const int*)before,
                           (const int*)gene_line, (const int*)R.start, g, k0, v0);
        HIPTRY(seg::sort_pairs(mem, k0, k1, v0, v1, g, 32 + seg::bits_for(contigs), &key_out, &val_out, s));
    } else {
        HIPTRY(hipEventRecord(h->ev[stage++], s));
    }
    HIPTRY(hipEventRecord(h->ev[stage++], s));
    Sorted& S = h->out;
    HIPTRY(mem.alloc(&S.file, (size_t)g));
    HIPTRY(mem.alloc(&S.start, (size_t)g));
    HIPTRY(mem.alloc(&S.end, (size_t)g));
    HIPTRY(mem.alloc(&S.fam, (size_t)g));
    HIPTRY(mem.alloc(&S.contig, (size_t)g));
    HIPTRY(mem.alloc(&S.span_off, (size_t)g * kGffSpans));
    HIPTRY(mem.alloc(&S.span_len, (size_t)g * kGffSpans));
    if (g) hipLaunchKernelGGL(k_gather, dim3(seg::blocks(g)), dim3(kThreads), 0, s, key_out, val_out, (const int*)gene_line, R, nl, g, S);
    hipLaunchKernelGGL(k_fasta_off, dim3(seg::blocks(nf)), dim3(kThreads), 0, s, B, (const int*)fasta_line, h->fasta_off);
    HIPTRY(hipGetLastError());
    HIPTRY(hipMemcpyAsync(error_out, error, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPTRY(hipEventRecord(h->ev[stage++], s));
    HIPTRY(hipStreamSynchronize(s));
    h->g = g;
    h->contigs = contigs;
    return hipSuccess;
}

}  // namespace

int nemgpu_gff_info(int* tile_bytes, int* n_thresholds, int* thresholds)
{
    (void)thresholds;                                      // (one radix sort for every contig size: there are none)
    if (tile_bytes) *tile_bytes = kGffTile;
    if (n_thresholds) *n_thresholds = 0;
    return NEMGPU_OK;
}

int nemgpu_gff_create(nemgpu_gff** out, int device, const char* families_text, long long bytes, int hash_bits, int* n_families)
{
    if (!out) return NEMGPU_E_FUNCARG;
    *out = nullptr;
    if (bytes < 0 || (bytes > 0 && !families_text) || bytes > INT_MAX - 64 || hash_bits < 0 || hash_bits > 64) {
        set_error("nemgpu_gff_create: the families table's text (below 2 GiB) and hash_bits in 0 .. 64 are needed"); return NEMGPU_E_FUNCARG;
    }
    note_hip_used();
    HIPCHK(hipSetDevice(device));
    nemgpu_gff* h = new nemgpu_gff();
    h->device = device;
    h->keep = hash_bits == 0 || hash_bits == 64 ? ~0ull : (1ull << hash_bits) - 1;
    hipError_t err = hipStreamCreate(&h->stream);
    for (int j = 0; err == hipSuccess && j <= kGffStages; j++) err = hipEventCreate(&h->ev[j]);
    if (err == hipSuccess) err = build_families(h, families_text, bytes);
    if (err != hipSuccess) { gff_free(h); return device_status("nemgpu_gff_create", err); }
    if (n_families) *n_families = h->n_families;
    *out = h;
    return NEMGPU_OK;
}

int nemgpu_gff_family_spans(const nemgpu_gff* h, int32_t* spans)
{
    if (!h || !spans) return NEMGPU_E_FUNCARG;
    std::copy(h->family_spans.begin(), h->family_spans.end(), spans);
    return NEMGPU_OK;
}

int nemgpu_gff_batch(nemgpu_gff* h, const char* text, long long bytes, const int32_t* file_start, const int32_t* file_end, int n_files,
                     int infer_singletons, int* n_genes, int* n_contigs, unsigned long long* error)
{
    if (!h || !file_start || !file_end || !n_genes || !n_contigs || !error) return NEMGPU_E_FUNCARG;
    const std::string who = "nemgpu_gff_batch";
    if (n_files <= 0 || n_files >= (1 << 23) || bytes < 0 || bytes > INT_MAX - 64 || (bytes > 0 && !text)) {
        set_error(who + ": between 1 and 2^23 files and less than 2 GiB of text are needed"); return NEMGPU_E_ARG;
    }
    for (int f = 0; f < n_files; f++) {                    // whole files in order, one byte between two of them
        const bool ok = file_start[f] >= 0 && file_end[f] >= file_start[f] && file_end[f] <= bytes &&
                        (f == 0 ? file_start[f] == 0 : file_start[f] == file_end[f - 1] + 1) && (f + 1 < n_files || file_end[f] == bytes);
        if (!ok) { set_error(who + ": the files are [start, end) in order from 0 to the text's end, a joint byte between two"); return NEMGPU_E_ARG; }
        if (f > 0 && text[file_start[f] - 1] != '\n') { set_error(who + ": the byte between two files is '\\n'"); return NEMGPU_E_ARG; }
    }
    HIPCHK(hipSetDevice(h->device));
    const hipError_t err = run_batch(h, text, bytes, file_start, file_end, n_files, infer_singletons, error);
    if (err != hipSuccess) { h->batch.reset(); h->g = h->contigs = 0; return device_status(who, err); }
    for (int j = 0; j < kGffStages; j++) (void)hipEventElapsedTime(&h->stage_ms[j], h->ev[j], h->ev[j + 1]);
    *n_genes = h->g;
    *n_contigs = h->contigs;
    return NEMGPU_OK;
}

int nemgpu_gff_fetch(const nemgpu_gff* h, int32_t* file, int32_t* start, int32_t* end, int32_t* span_off, int32_t* span_len, int32_t* fam,
                     int32_t* contig, int32_t* fasta_off)
{
    if (!h) return NEMGPU_E_FUNCARG;
    if (!h->batch) { set_error("nemgpu_gff_fetch: no batch has been run"); return NEMGPU_E_ARG; }
    HIPCHK(hipSetDevice(h->device));
    const size_t g = (size_t)h->g;
    const Sorted& S = h->out;
    if (g) {
        if (file) HIPCHK(hipMemcpy(file, S.file, g * 4, hipMemcpyDeviceToHost));
        if (start) HIPCHK(hipMemcpy(start, S.start, g * 4, hipMemcpyDeviceToHost));
        if (end) HIPCHK(hipMemcpy(end, S.end, g * 4, hipMemcpyDeviceToHost));
        if (span_off) HIPCHK(hipMemcpy(span_off, S.span_off, g * 4 * kGffSpans, hipMemcpyDeviceToHost));
        if (span_len) HIPCHK(hipMemcpy(span_len, S.span_len, g * 4 * kGffSpans, hipMemcpyDeviceToHost));
        if (fam) HIPCHK(hipMemcpy(fam, S.fam, g * 4, hipMemcpyDeviceToHost));
        if (contig) HIPCHK(hipMemcpy(contig, S.contig, g * 4, hipMemcpyDeviceToHost));
    }
    if (fasta_off) HIPCHK(hipMemcpy(fasta_off, h->fasta_off, (size_t)h->files * 4, hipMemcpyDeviceToHost));
    return NEMGPU_OK;
}

int nemgpu_gff_number(nemgpu_gff* h, const int32_t* name, const int32_t* org, int g, int n_names, int n_orgs, int lim_occurence, int32_t* genes,
                      int32_t* order, uint8_t* repeated, int* n_used)
{
    if (!h || !n_used || (g > 0 && (!name || !org || !genes || !order)) || !repeated) return NEMGPU_E_FUNCARG;
    const std::string who = "nemgpu_gff_number";
    if (g < 0 || g > (1 << 30) || n_names < 0 || n_orgs < 0) { set_error(who + ": at most 2^30 genes"); return NEMGPU_E_ARG; }
    for (int p = 0; p < g; p++) {
        if (name[p] < 0 || name[p] >= n_names || org[p] < 0 || org[p] >= n_orgs) { set_error(who + ": a name or an organism out of range"); return NEMGPU_E_ARG; }
    }
    *n_used = 0;
    repeated[0] = 0;
    if (g == 0) return NEMGPU_OK;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    seg::Scratch mem;
    int used = 0;
    const auto run = [&]() -> hipError_t {
        int *d_name, *d_org, *first, *head, *before, *d_genes, *d_order;
        uint64_t *k0, *k1;
        uint8_t* d_rep;
        HIPTRY(mem.alloc(&d_name, (size_t)g));
        HIPTRY(mem.alloc(&d_org, (size_t)g));
        HIPTRY(mem.alloc(&first, (size_t)n_names));
        HIPTRY(mem.alloc(&head, (size_t)g));
        HIPTRY(mem.alloc(&d_genes, (size_t)g));
        HIPTRY(mem.alloc(&d_order, (size_t)n_names));
        HIPTRY(mem.alloc(&k0, (size_t)g));
        HIPTRY(mem.alloc(&k1, (size_t)g));
        HIPTRY(mem.alloc(&d_rep, (size_t)n_names));
        HIPTRY(hipMemcpyAsync(d_name, name, (size_t)g * 4, hipMemcpyHostToDevice, s));
        HIPTRY(hipMemcpyAsync(d_org, org, (size_t)g * 4, hipMemcpyHostToDevice, s));
        HIPTRY(hipMemsetAsync(first, 0x7F, (size_t)n_names * 4, s));       // (0x7F7F7F7F: above every position)
        HIPTRY(hipMemsetAsync(d_rep, 0, (size_t)n_names, s));
        const int nb = seg::blocks(g);
        hipLaunchKernelGGL(k_first_gene, dim3(nb), dim3(kThreads), 0, s, (const int*)d_name, g, first);
        hipLaunchKernelGGL(k_first_flags, dim3(nb), dim3(kThreads), 0, s, (const int*)d_name, (const int*)first, g, head);
        HIPTRY(ranks(mem, head, g, &before, &used, s));
        hipLaunchKernelGGL(k_family_ids, dim3(nb), dim3(kThreads), 0, s, (const int*)d_name, (const int*)first, (const int*)head, (const int*)before,
                           (const int*)d_org, g, d_genes, d_order, k0);
        if (lim_occurence > 0 && lim_occurence < g) {
            const uint64_t* sorted = nullptr;
            HIPTRY(seg::sort_keys(mem, k0, k1, g, 32 + seg::bits_for(n_orgs), &sorted, s));
            hipLaunchKernelGGL(k_repeated, dim3(nb), dim3(kThreads), 0, s, sorted, g, lim_occurence, d_rep);
        }
        HIPTRY(hipGetLastError());
        HIPTRY(hipMemcpyAsync(genes, d_genes, (size_t)g * 4, hipMemcpyDeviceToHost, s));
        HIPTRY(hipMemcpyAsync(order, d_order, (size_t)used * 4, hipMemcpyDeviceToHost, s));
        HIPTRY(hipMemcpyAsync(repeated, d_rep, (size_t)used, hipMemcpyDeviceToHost, s));
        return hipStreamSynchronize(s);
    };
    const hipError_t err = run();
    if (err != hipSuccess) return device_status(who, err);
    *n_used = used;
    return NEMGPU_OK;
}

int nemgpu_gff_stage_ms(const nemgpu_gff* h, float* ms)
{
    if (!h || !ms) return NEMGPU_E_FUNCARG;
    for (int j = 0; j < kGffStages; j++) ms[j] = h->stage_ms[j];
    return NEMGPU_OK;
}

void nemgpu_gff_destroy(nemgpu_gff* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    gff_free(h);
}
