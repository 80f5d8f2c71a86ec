/* wirehead: see wirehead.h. Mirrors, for the inputs it accepts, the head
 * parsing of active_monitor_amd/utils/wirecodec.py (_py_parse_request_head,
 * _py_parse_response_head); everything else is AM_HEAD_BAIL.
 *
 * Accepted bytes are printable ASCII (0x20..0x7e) plus CR LF pairs as line
 * ends. With that, bytes.strip() can only ever remove spaces, bytes.lower()
 * only touches A-Z, and latin-1 decoding is the identity, which is what
 * makes the equivalence easy to see.
 */
#include "wirehead.h"

#include <string.h>

/* Next CRLF-terminated line starting at *pos. Returns 0 when the bytes up
 * to the line end are not all acceptable or no CRLF follows. */
static int
next_line(const char *buf, size_t len, size_t *pos, am_span *line)
{
    size_t i = *pos;
    while (i < len) {
        unsigned char c = (unsigned char)buf[i];
        if (c == '\r') {
            if (i + 1 >= len || buf[i + 1] != '\n')
                return 0;
            line->p = buf + *pos;
            line->n = i - *pos;
            *pos = i + 2;
            return 1;
        }
        if (c < 0x20 || c > 0x7e)
            return 0;
        i++;
    }
    return 0;
}

static int
lower(int c)
{
    return (c >= 'A' && c <= 'Z') ? c + 32 : c;
}

/* lit is lower-case */
static int
ci_prefix(am_span s, const char *lit)
{
    size_t n = strlen(lit);
    if (s.n < n)
        return 0;
    for (size_t i = 0; i < n; i++)
        if (lower((unsigned char)s.p[i]) != lit[i])
            return 0;
    return 1;
}

static int
ci_contains(am_span s, const char *lit)
{
    size_t n = strlen(lit);
    if (s.n < n)
        return 0;
    for (size_t i = 0; i + n <= s.n; i++) {
        size_t j = 0;
        while (j < n && lower((unsigned char)s.p[i + j]) == lit[j])
            j++;
        if (j == n)
            return 1;
    }
    return 0;
}

/* the stripped text after the first n bytes (the "name:" prefix) */
static am_span
value_after(am_span line, size_t n)
{
    am_span v = {line.p + n, line.n - n};
    while (v.n > 0 && v.p[0] == ' ') {
        v.p++;
        v.n--;
    }
    while (v.n > 0 && v.p[v.n - 1] == ' ')
        v.n--;
    return v;
}

/* 1..18 plain digits; anything int() would treat specially bails */
static int
plain_digits(am_span v, long long *out)
{
    if (v.n == 0 || v.n > 18)
        return 0;
    long long x = 0;
    for (size_t i = 0; i < v.n; i++) {
        if (v.p[i] < '0' || v.p[i] > '9')
            return 0;
        x = x * 10 + (v.p[i] - '0');
    }
    *out = x;
    return 1;
}

int
am_parse_request_head(const char *buf, size_t len, am_request_head *out)
{
    size_t pos = 0;
    am_span line;
    memset(out, 0, sizeof(*out));
    out->content_type.p = out->authorization.p = buf;
    if (!next_line(buf, len, &pos, &line))
        return AM_HEAD_BAIL;

    /* METHOD SP TARGET SP HTTP/... */
    size_t i = 0;
    while (i < line.n && line.p[i] >= 'A' && line.p[i] <= 'Z')
        i++;
    if (i == 0 || i > 16 || i >= line.n || line.p[i] != ' ')
        return AM_HEAD_BAIL;
    out->method.p = line.p;
    out->method.n = i;
    size_t t0 = ++i;
    size_t qmark = 0;
    int has_q = 0;
    while (i < line.n && line.p[i] != ' ') {
        char c = line.p[i];
        if (c == '%' || c == '+' || c == '#')
            return AM_HEAD_BAIL;
        if (c == '?' && !has_q) {
            has_q = 1;
            qmark = i;
        }
        i++;
    }
    /* origin-form only: "/x", never "//x" (a netloc to urlsplit) */
    if (i == t0 || line.p[t0] != '/' || (i > t0 + 1 && line.p[t0 + 1] == '/'))
        return AM_HEAD_BAIL;
    if (i + 6 > line.n || memcmp(line.p + i, " HTTP/", 6) != 0)
        return AM_HEAD_BAIL;
    out->path.p = line.p + t0;
    if (has_q) {
        out->path.n = qmark - t0;
        out->query.p = line.p + qmark + 1;
        out->query.n = i - qmark - 1;
    } else {
        out->path.n = i - t0;
        out->query.p = line.p + i;
        out->query.n = 0;
    }

    for (;;) {
        if (!next_line(buf, len, &pos, &line))
            return AM_HEAD_BAIL;
        if (line.n == 0)
            break;
        if (ci_prefix(line, "content-length:")) {
            if (!plain_digits(value_after(line, 15), &out->content_length))
                return AM_HEAD_BAIL;
        } else if (ci_prefix(line, "content-type:")) {
            out->content_type = value_after(line, 13);
        } else if (ci_prefix(line, "expect:")) {
            if (ci_contains(line, "100-continue"))
                out->flags |= AM_FLAG_EXPECT_CONTINUE;
        } else if (ci_prefix(line, "accept:")) {
            if (ci_contains(line, "as=table"))
                out->flags |= AM_FLAG_WANT_TABLE;
        } else if (ci_prefix(line, "authorization:")) {
            out->authorization = value_after(line, 14);
        }
    }
    /* the blank line must be the end of what was handed in */
    return pos == len ? AM_HEAD_OK : AM_HEAD_BAIL;
}

int
am_parse_response_head(const char *buf, size_t len, am_response_head *out)
{
    size_t pos = 0;
    am_span line;
    memset(out, 0, sizeof(*out));
    out->keep_alive = 1;
    if (!next_line(buf, len, &pos, &line))
        return AM_HEAD_BAIL;

    /* HTTP/x.y SP ddd [SP reason] */
    if (line.n < 5 || memcmp(line.p, "HTTP/", 5) != 0)
        return AM_HEAD_BAIL;
    size_t i = 5;
    while (i < line.n && line.p[i] != ' ')
        i++;
    if (i + 4 > line.n)
        return AM_HEAD_BAIL;
    int status = 0;
    for (size_t k = i + 1; k < i + 4; k++) {
        if (line.p[k] < '0' || line.p[k] > '9')
            return AM_HEAD_BAIL;
        status = status * 10 + (line.p[k] - '0');
    }
    if (i + 4 < line.n && line.p[i + 4] != ' ')
        return AM_HEAD_BAIL;
    out->status = status;

    for (;;) {
        if (!next_line(buf, len, &pos, &line))
            return AM_HEAD_BAIL;
        if (line.n == 0)
            break;
        if (ci_prefix(line, "content-length:")) {
            if (!plain_digits(value_after(line, 15), &out->content_length))
                return AM_HEAD_BAIL;
        } else if (ci_prefix(line, "transfer-encoding:")) {
            if (ci_contains(line, "chunked"))
                out->chunked = 1;
        } else if (ci_prefix(line, "connection:")) {
            if (ci_contains(line, "close"))
                out->keep_alive = 0;
        }
    }
    return pos == len ? AM_HEAD_OK : AM_HEAD_BAIL;
}

int
am_query_next(const char *q, size_t len, size_t *pos,
              am_span *name, am_span *value)
{
    while (*pos < len) {
        size_t start = *pos, i = start, eq = 0;
        int has_eq = 0;
        while (i < len && q[i] != '&') {
            if (q[i] == '=' && !has_eq) {
                has_eq = 1;
                eq = i;
            }
            i++;
        }
        *pos = i < len ? i + 1 : len;
        if (!has_eq || eq + 1 == i)
            continue; /* no '=' or blank value: parse_qsl drops it */
        name->p = q + start;
        name->n = eq - start;
        value->p = q + eq + 1;
        value->n = i - eq - 1;
        return 1;
    }
    return 0;
}
