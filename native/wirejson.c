/* wirejson: the JSON codec of the wire path.
 *
 *   json_dumpb(obj)          compact JSON as bytes, byte-identical to
 *                            json.dumps(obj, separators=(",", ":")).encode()
 *   json_frame(prefix, obj)  prefix + "Content-Length: n\r\n\r\n" + payload
 *                            in one bytes object (obj None: empty payload)
 *   json_loadb(data)         parse UTF-8 JSON from a bytes-like object
 *
 * Same pattern as deep_copy/snapshot: a narrow fast path for the shapes the
 * wire carries - exact dict (str keys)/list/tuple/str/int/float/bool/None -
 * and NotImplemented for everything else, on which the caller runs the
 * stdlib expression unchanged. Nothing here raises: any failure, including
 * an exhausted recursion budget, is turned into NotImplemented so that the
 * stdlib produces the value or the exception it always produced.
 */
#include "wirejson.h"

#include <string.h>

/* ------------------------------------------------------------------ */
/* encoder                                                             */

typedef struct {
    char *buf;
    size_t len, cap;
} wbuf;

static int
wb_grow(wbuf *w, size_t extra)
{
    size_t need = w->len + extra;
    size_t cap = w->cap * 2;
    if (cap < need)
        cap = need;
    char *nb = PyMem_Realloc(w->buf, cap);
    if (nb == NULL)
        return -1;
    w->buf = nb;
    w->cap = cap;
    return 0;
}

#define WB_RESERVE(w, extra) \
    (((w)->len + (size_t)(extra) <= (w)->cap) ? 0 : wb_grow((w), (size_t)(extra)))

static int
wb_put(wbuf *w, const char *s, size_t n)
{
    if (WB_RESERVE(w, n) < 0)
        return -1;
    memcpy(w->buf + w->len, s, n);
    w->len += n;
    return 0;
}

static const char HEX[] = "0123456789abcdef";

static char *
put_u16(char *o, unsigned v)
{
    *o++ = '\\';
    *o++ = 'u';
    *o++ = HEX[(v >> 12) & 15];
    *o++ = HEX[(v >> 8) & 15];
    *o++ = HEX[(v >> 4) & 15];
    *o++ = HEX[v & 15];
    return o;
}

/* the ensure_ascii escape of one character that needs one; at most 12 bytes */
static char *
put_escape(char *o, Py_UCS4 c)
{
    switch (c) {
    case '"': *o++ = '\\'; *o++ = '"'; return o;
    case '\\': *o++ = '\\'; *o++ = '\\'; return o;
    case '\b': *o++ = '\\'; *o++ = 'b'; return o;
    case '\f': *o++ = '\\'; *o++ = 'f'; return o;
    case '\n': *o++ = '\\'; *o++ = 'n'; return o;
    case '\r': *o++ = '\\'; *o++ = 'r'; return o;
    case '\t': *o++ = '\\'; *o++ = 't'; return o;
    }
    if (c >= 0x10000) {
        Py_UCS4 v = c - 0x10000;
        o = put_u16(o, 0xd800 | ((v >> 10) & 0x3ff));
        return put_u16(o, 0xdc00 | (v & 0x3ff));
    }
    return put_u16(o, (unsigned)c);
}

/* what ensure_ascii copies through: ' '..'~' but the two below; 0x7f is
 * escaped like every other non-printable */
#define PLAIN(c) ((c) >= 0x20 && (c) < 0x7f && (c) != '"' && (c) != '\\')

static int
enc_str(wbuf *w, PyObject *s)
{
    if (PyUnicode_READY(s) < 0)
        return -1;
    Py_ssize_t n = PyUnicode_GET_LENGTH(s);
    int kind = PyUnicode_KIND(s);
    const void *data = PyUnicode_DATA(s);
    /* invariant below: room for the unwritten characters as plain bytes
     * plus the closing quote; every escape reserves its own 12 on top */
    if (WB_RESERVE(w, (size_t)n + 2) < 0)
        return -1;
    w->buf[w->len++] = '"';
    if (kind == PyUnicode_1BYTE_KIND) {
        const unsigned char *d = data;
        Py_ssize_t i = 0;
        while (i < n) {
            Py_ssize_t j = i;
            while (j < n && PLAIN(d[j]))
                j++;
            memcpy(w->buf + w->len, d + i, (size_t)(j - i));
            w->len += (size_t)(j - i);
            if (j == n)
                break;
            if (WB_RESERVE(w, (size_t)(n - j) + 13) < 0)
                return -1;
            w->len = (size_t)(put_escape(w->buf + w->len, d[j]) - w->buf);
            i = j + 1;
        }
    } else {
        for (Py_ssize_t i = 0; i < n; i++) {
            Py_UCS4 c = PyUnicode_READ(kind, data, i);
            if (PLAIN(c)) {
                w->buf[w->len++] = (char)c;
            } else {
                if (WB_RESERVE(w, (size_t)(n - i) + 13) < 0)
                    return -1;
                w->len = (size_t)(put_escape(w->buf + w->len, c) - w->buf);
            }
        }
    }
    w->buf[w->len++] = '"';
    return 0;
}

static int
enc_int(wbuf *w, PyObject *o)
{
    int overflow = 0;
    long long v = PyLong_AsLongLongAndOverflow(o, &overflow);
    if (!overflow) {
        if (v == -1 && PyErr_Occurred())
            return -1;
        char tmp[24];
        char *p = tmp + sizeof(tmp);
        unsigned long long u = v < 0 ? 0ULL - (unsigned long long)v
                                     : (unsigned long long)v;
        do {
            *--p = (char)('0' + u % 10);
            u /= 10;
        } while (u);
        if (v < 0)
            *--p = '-';
        return wb_put(w, p, (size_t)(tmp + sizeof(tmp) - p));
    }
    PyObject *r = PyLong_Type.tp_repr(o);
    if (r == NULL)
        return -1;
    Py_ssize_t n;
    const char *s = PyUnicode_AsUTF8AndSize(r, &n);
    int rc = s == NULL ? -1 : wb_put(w, s, (size_t)n);
    Py_DECREF(r);
    return rc;
}

static int
enc_float(wbuf *w, PyObject *o)
{
    double d = PyFloat_AS_DOUBLE(o);
    if (!Py_IS_FINITE(d))
        return -1; /* NaN/Infinity spellings are the stdlib's business */
    char *s = PyOS_double_to_string(d, 'r', 0, Py_DTSF_ADD_DOT_0, NULL);
    if (s == NULL)
        return -1;
    int rc = wb_put(w, s, strlen(s));
    PyMem_Free(s);
    return rc;
}

/* 0 = written, -1 = not handled (an exception may be set; callers clear) */
static int
enc_value(wbuf *w, PyObject *o)
{
    if (PyUnicode_CheckExact(o))
        return enc_str(w, o);
    if (o == Py_None)
        return wb_put(w, "null", 4);
    if (o == Py_True)
        return wb_put(w, "true", 4);
    if (o == Py_False)
        return wb_put(w, "false", 5);
    if (PyLong_CheckExact(o))
        return enc_int(w, o);
    if (PyFloat_CheckExact(o))
        return enc_float(w, o);

    int rc = -1;
    if (PyDict_CheckExact(o)) {
        if (Py_EnterRecursiveCall(" while encoding a JSON object"))
            return -1;
        Py_ssize_t pos = 0;
        PyObject *key, *value;
        int first = 1;
        rc = wb_put(w, "{", 1);
        while (rc == 0 && PyDict_Next(o, &pos, &key, &value)) {
            if (!PyUnicode_CheckExact(key)) {
                rc = -1;
                break;
            }
            if (!first)
                rc = wb_put(w, ",", 1);
            first = 0;
            if (rc == 0)
                rc = enc_str(w, key);
            if (rc == 0)
                rc = wb_put(w, ":", 1);
            if (rc == 0)
                rc = enc_value(w, value);
        }
        if (rc == 0)
            rc = wb_put(w, "}", 1);
        Py_LeaveRecursiveCall();
    } else if (PyList_CheckExact(o) || PyTuple_CheckExact(o)) {
        if (Py_EnterRecursiveCall(" while encoding a JSON object"))
            return -1;
        int is_list = PyList_CheckExact(o);
        rc = wb_put(w, "[", 1);
        /* the size is re-read every round; nothing below runs Python code,
         * this is only belt and braces */
        for (Py_ssize_t i = 0; rc == 0 && i < Py_SIZE(o); i++) {
            if (i)
                rc = wb_put(w, ",", 1);
            if (rc == 0)
                rc = enc_value(w, is_list ? PyList_GET_ITEM(o, i)
                                          : PyTuple_GET_ITEM(o, i));
        }
        if (rc == 0)
            rc = wb_put(w, "]", 1);
        Py_LeaveRecursiveCall();
    }
    return rc;
}

static PyObject *
not_handled(void)
{
    PyErr_Clear();
    Py_RETURN_NOTIMPLEMENTED;
}

PyObject *
am_json_dumpb(PyObject *self, PyObject *obj)
{
    (void)self;
    wbuf w = {PyMem_Malloc(2048), 0, 2048};
    if (w.buf == NULL)
        return PyErr_NoMemory();
    PyObject *out;
    if (enc_value(&w, obj) < 0)
        out = not_handled();
    else
        out = PyBytes_FromStringAndSize(w.buf, (Py_ssize_t)w.len);
    PyMem_Free(w.buf);
    return out;
}

#define FRAME_HEAD_MAX 48 /* "Content-Length: " + 20 digits + CRLF CRLF */

PyObject *
am_json_frame(PyObject *self, PyObject *const *args, Py_ssize_t nargs)
{
    (void)self;
    if (nargs != 2 || !PyBytes_Check(args[0])) {
        PyErr_SetString(PyExc_TypeError, "json_frame(prefix: bytes, obj)");
        return NULL;
    }
    size_t plen = (size_t)PyBytes_GET_SIZE(args[0]);
    /* the payload is encoded behind a gap that the prefix and the
     * Content-Length line are then written into, right-aligned */
    size_t gap = plen + FRAME_HEAD_MAX;
    wbuf w = {PyMem_Malloc(gap + 2048), gap, gap + 2048};
    if (w.buf == NULL)
        return PyErr_NoMemory();
    PyObject *out;
    if (args[1] != Py_None && enc_value(&w, args[1]) < 0) {
        out = not_handled();
    } else {
        char head[FRAME_HEAD_MAX];
        int hl = PyOS_snprintf(head, sizeof(head), "Content-Length: %zu\r\n\r\n",
                               w.len - gap);
        char *start = w.buf + gap - (size_t)hl - plen;
        memcpy(start, PyBytes_AS_STRING(args[0]), plen);
        memcpy(start + plen, head, (size_t)hl);
        out = PyBytes_FromStringAndSize(start, (Py_ssize_t)(w.buf + w.len - start));
    }
    PyMem_Free(w.buf);
    return out;
}

/* ------------------------------------------------------------------ */
/* decoder                                                             */

typedef struct {
    const unsigned char *p, *end;
} rbuf;

static PyObject *key_cache[AM_KEY_CACHE_SLOTS];

static PyObject *dec_value(rbuf *r);

static inline void
skip_ws(rbuf *r)
{
    while (r->p < r->end &&
           (*r->p == ' ' || *r->p == '\n' || *r->p == '\r' || *r->p == '\t'))
        r->p++;
}

static PyObject *
ascii_str(const unsigned char *s, size_t n)
{
    PyObject *u = PyUnicode_New((Py_ssize_t)n, 127);
    if (u != NULL)
        memcpy(PyUnicode_1BYTE_DATA(u), s, n);
    return u;
}

/* dict keys repeat forever on this wire: short ASCII keys are shared
 * through a direct-mapped cache, replaced on collision (GIL held) */
static PyObject *
cached_key(const unsigned char *s, size_t n)
{
    uint32_t h = 2166136261u;
    for (size_t i = 0; i < n; i++)
        h = (h ^ s[i]) * 16777619u;
    PyObject **slot = &key_cache[h % AM_KEY_CACHE_SLOTS];
    PyObject *e = *slot;
    if (e != NULL && (size_t)PyUnicode_GET_LENGTH(e) == n &&
        memcmp(PyUnicode_1BYTE_DATA(e), s, n) == 0) {
        Py_INCREF(e);
        return e;
    }
    PyObject *u = ascii_str(s, n);
    if (u == NULL)
        return NULL;
    Py_INCREF(u);
    *slot = u;
    Py_XDECREF(e);
    return u;
}

static int
hex4(const unsigned char *p, Py_UCS4 *out)
{
    Py_UCS4 v = 0;
    for (int i = 0; i < 4; i++) {
        unsigned char c = p[i];
        v <<= 4;
        if (c >= '0' && c <= '9')
            v |= (Py_UCS4)(c - '0');
        else if (c >= 'a' && c <= 'f')
            v |= (Py_UCS4)(c - 'a' + 10);
        else if (c >= 'A' && c <= 'F')
            v |= (Py_UCS4)(c - 'A' + 10);
        else
            return -1;
    }
    *out = v;
    return 0;
}

/* One strictly valid UTF-8 sequence with lead byte >= 0x80 from [p, end);
 * returns its length, 0 when invalid (overlong, surrogate, > U+10FFFF,
 * truncated). */
static int
utf8_one(const unsigned char *p, const unsigned char *end, Py_UCS4 *out)
{
    unsigned char c = p[0];
    int n;
    unsigned char lo = 0x80, hi = 0xbf;
    Py_UCS4 v;
    if (c >= 0xc2 && c <= 0xdf) {
        n = 2;
        v = c & 0x1f;
    } else if (c >= 0xe0 && c <= 0xef) {
        n = 3;
        v = c & 0x0f;
        if (c == 0xe0)
            lo = 0xa0;
        else if (c == 0xed)
            hi = 0x9f;
    } else if (c >= 0xf0 && c <= 0xf4) {
        n = 4;
        v = c & 0x07;
        if (c == 0xf0)
            lo = 0x90;
        else if (c == 0xf4)
            hi = 0x8f;
    } else {
        return 0;
    }
    if (end - p < n)
        return 0;
    if (p[1] < lo || p[1] > hi)
        return 0;
    v = (v << 6) | (p[1] & 0x3f);
    for (int i = 2; i < n; i++) {
        if (p[i] < 0x80 || p[i] > 0xbf)
            return 0;
        v = (v << 6) | (p[i] & 0x3f);
    }
    *out = v;
    return n;
}

/* string body [s, q) that holds at least one backslash */
static PyObject *
dec_escaped(const unsigned char *s, const unsigned char *q)
{
    Py_UCS4 stack[256];
    Py_UCS4 *out = stack;
    size_t cap = (size_t)(q - s); /* never more characters than bytes */
    if (cap > 256) {
        out = PyMem_Malloc(cap * sizeof(Py_UCS4));
        if (out == NULL)
            return NULL;
    }
    size_t n = 0;
    PyObject *res = NULL;
    while (s < q) {
        unsigned char c = *s;
        if (c >= 0x80) {
            Py_UCS4 v;
            int k = utf8_one(s, q, &v);
            if (k == 0)
                goto done;
            out[n++] = v;
            s += k;
        } else if (c != '\\') {
            out[n++] = c;
            s++;
        } else {
            if (q - s < 2)
                goto done;
            unsigned char e = s[1];
            s += 2;
            switch (e) {
            case '"': case '\\': case '/': out[n++] = e; break;
            case 'b': out[n++] = '\b'; break;
            case 'f': out[n++] = '\f'; break;
            case 'n': out[n++] = '\n'; break;
            case 'r': out[n++] = '\r'; break;
            case 't': out[n++] = '\t'; break;
            case 'u': {
                Py_UCS4 v, v2;
                if (q - s < 4 || hex4(s, &v) < 0)
                    goto done;
                s += 4;
                /* an escaped high surrogate joins an escaped low one that
                 * follows directly; otherwise it stands alone, as in the
                 * stdlib */
                if (v >= 0xd800 && v <= 0xdbff && q - s >= 6 &&
                    s[0] == '\\' && s[1] == 'u') {
                    if (hex4(s + 2, &v2) < 0)
                        goto done;
                    if (v2 >= 0xdc00 && v2 <= 0xdfff) {
                        v = 0x10000 + (((v - 0xd800) << 10) | (v2 - 0xdc00));
                        s += 6;
                    }
                }
                out[n++] = v;
                break;
            }
            default:
                goto done;
            }
        }
    }
    res = PyUnicode_FromKindAndData(PyUnicode_4BYTE_KIND, out, (Py_ssize_t)n);
done:
    if (out != stack)
        PyMem_Free(out);
    return res;
}

/* r->p is at the opening quote */
static PyObject *
dec_string(rbuf *r, int is_key)
{
    const unsigned char *s = r->p + 1, *q = s, *end = r->end;
    int escaped = 0;
    unsigned char high = 0;
    for (;;) {
        if (q >= end)
            return NULL;
        unsigned char c = *q;
        if (c == '"')
            break;
        if (c == '\\') {
            escaped = 1;
            q += 2;
            continue;
        }
        if (c < 0x20)
            return NULL;
        high |= c;
        q++;
    }
    r->p = q + 1;
    size_t n = (size_t)(q - s);
    if (escaped)
        return dec_escaped(s, q);
    if (high & 0x80) /* strict: rejects what the stdlib treats specially */
        return PyUnicode_DecodeUTF8((const char *)s, (Py_ssize_t)n, NULL);
    if (is_key && n <= AM_KEY_CACHE_MAX_LEN)
        return cached_key(s, n);
    return ascii_str(s, n);
}

static PyObject *
dec_number(rbuf *r)
{
    const unsigned char *s = r->p, *p = s, *end = r->end;
    int neg = 0, is_float = 0;
    if (*p == '-') {
        neg = 1;
        p++;
    }
    const unsigned char *digits = p;
    if (p >= end)
        return NULL;
    if (*p == '0') {
        p++;
        if (p < end && *p >= '0' && *p <= '9')
            return NULL;
    } else if (*p >= '1' && *p <= '9') {
        while (p < end && *p >= '0' && *p <= '9')
            p++;
    } else {
        return NULL;
    }
    size_t nint = (size_t)(p - digits);
    if (p < end && *p == '.') {
        p++;
        if (p >= end || *p < '0' || *p > '9')
            return NULL;
        while (p < end && *p >= '0' && *p <= '9')
            p++;
        is_float = 1;
    }
    if (p < end && (*p == 'e' || *p == 'E')) {
        p++;
        if (p < end && (*p == '+' || *p == '-'))
            p++;
        if (p >= end || *p < '0' || *p > '9')
            return NULL;
        while (p < end && *p >= '0' && *p <= '9')
            p++;
        is_float = 1;
    }
    r->p = p;
    if (!is_float && nint <= 18) {
        long long v = 0;
        for (size_t i = 0; i < nint; i++)
            v = v * 10 + (digits[i] - '0');
        return PyLong_FromLongLong(neg ? -v : v);
    }
    /* the literal, NUL-terminated, for the two CPython converters */
    char stack[64];
    size_t n = (size_t)(p - s);
    char *lit = n < sizeof(stack) ? stack : PyMem_Malloc(n + 1);
    if (lit == NULL)
        return NULL;
    memcpy(lit, s, n);
    lit[n] = '\0';
    PyObject *res = NULL;
    if (is_float) {
        double d = PyOS_string_to_double(lit, NULL, NULL);
        if (!(d == -1.0 && PyErr_Occurred()))
            res = PyFloat_FromDouble(d);
    } else {
        res = PyLong_FromString(lit, NULL, 10);
    }
    if (lit != stack)
        PyMem_Free(lit);
    return res;
}

static int
literal(rbuf *r, const char *word, size_t n)
{
    if ((size_t)(r->end - r->p) < n || memcmp(r->p, word, n) != 0)
        return 0;
    r->p += n;
    return 1;
}

static PyObject *
dec_object(rbuf *r)
{
    PyObject *d = PyDict_New();
    if (d == NULL)
        return NULL;
    r->p++;
    skip_ws(r);
    if (r->p < r->end && *r->p == '}') {
        r->p++;
        return d;
    }
    for (;;) {
        if (r->p >= r->end || *r->p != '"')
            goto fail;
        PyObject *key = dec_string(r, 1);
        if (key == NULL)
            goto fail;
        skip_ws(r);
        if (r->p >= r->end || *r->p != ':') {
            Py_DECREF(key);
            goto fail;
        }
        r->p++;
        skip_ws(r);
        PyObject *val = dec_value(r);
        if (val == NULL) {
            Py_DECREF(key);
            goto fail;
        }
        int rc = PyDict_SetItem(d, key, val); /* duplicate key: last wins */
        Py_DECREF(key);
        Py_DECREF(val);
        if (rc < 0)
            goto fail;
        skip_ws(r);
        if (r->p >= r->end)
            goto fail;
        if (*r->p == '}') {
            r->p++;
            return d;
        }
        if (*r->p != ',')
            goto fail;
        r->p++;
        skip_ws(r);
    }
fail:
    Py_DECREF(d);
    return NULL;
}

static PyObject *
dec_array(rbuf *r)
{
    PyObject *l = PyList_New(0);
    if (l == NULL)
        return NULL;
    r->p++;
    skip_ws(r);
    if (r->p < r->end && *r->p == ']') {
        r->p++;
        return l;
    }
    for (;;) {
        PyObject *val = dec_value(r);
        if (val == NULL)
            goto fail;
        int rc = PyList_Append(l, val);
        Py_DECREF(val);
        if (rc < 0)
            goto fail;
        skip_ws(r);
        if (r->p >= r->end)
            goto fail;
        if (*r->p == ']') {
            r->p++;
            return l;
        }
        if (*r->p != ',')
            goto fail;
        r->p++;
        skip_ws(r);
    }
fail:
    Py_DECREF(l);
    return NULL;
}

/* NULL = not handled (an exception may be set; the entry point clears) */
static PyObject *
dec_value(rbuf *r)
{
    if (r->p >= r->end)
        return NULL;
    PyObject *res;
    switch (*r->p) {
    case '"':
        return dec_string(r, 0);
    case '{':
        if (Py_EnterRecursiveCall(" while decoding a JSON object"))
            return NULL;
        res = dec_object(r);
        Py_LeaveRecursiveCall();
        return res;
    case '[':
        if (Py_EnterRecursiveCall(" while decoding a JSON array"))
            return NULL;
        res = dec_array(r);
        Py_LeaveRecursiveCall();
        return res;
    case 't':
        if (literal(r, "true", 4))
            Py_RETURN_TRUE;
        return NULL;
    case 'f':
        if (literal(r, "false", 5))
            Py_RETURN_FALSE;
        return NULL;
    case 'n':
        if (literal(r, "null", 4))
            Py_RETURN_NONE;
        return NULL;
    case '-': case '0': case '1': case '2': case '3': case '4':
    case '5': case '6': case '7': case '8': case '9':
        return dec_number(r);
    }
    return NULL;
}

PyObject *
am_json_loadb(PyObject *self, PyObject *data)
{
    (void)self;
    Py_buffer view;
    if (PyObject_GetBuffer(data, &view, PyBUF_SIMPLE) < 0)
        return not_handled();
    rbuf r = {view.buf, (const unsigned char *)view.buf + view.len};
    skip_ws(&r);
    PyObject *res = dec_value(&r);
    if (res != NULL) {
        skip_ws(&r);
        if (r.p != r.end)
            Py_CLEAR(res); /* trailing garbage */
    }
    PyBuffer_Release(&view);
    if (res == NULL)
        return not_handled();
    return res;
}
