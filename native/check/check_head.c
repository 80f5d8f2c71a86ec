/* check_head: memory-safety run of the head parsers (native/wirehead.c),
 * built with -fsanitize=address,undefined by `make native-check`.
 *
 * Every input is copied into a heap block of exactly its length, so a read
 * one byte past the head is a sanitizer report. The only assertions are:
 * no report, the result is OK or BAIL, and on OK every span lies inside the
 * input. What the parsers answer is the business of
 * tests/unit/test_wirecodec_head.py.
 */
#include "wirehead.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static unsigned long runs, handled;

static void
die(const char *what, const char *buf, size_t len)
{
    fprintf(stderr, "check_head: %s on input of %zu bytes: ", what, len);
    fwrite(buf, 1, len < 200 ? len : 200, stderr);
    fputc('\n', stderr);
    exit(1);
}

static void
inside(am_span s, const char *buf, size_t len, const char *orig)
{
    if (s.p < buf || s.p > buf + len || s.n > (size_t)(buf + len - s.p))
        die("span outside the input", orig, len);
}

static void
feed(const char *data, size_t len)
{
    /* malloc(0) may return NULL; one spare byte block keeps p valid while
     * the parsers are still told len bytes */
    char *buf = malloc(len ? len : 1);
    if (buf == NULL)
        abort();
    memcpy(buf, data, len);

    am_request_head rq;
    int rc = am_parse_request_head(buf, len, &rq);
    if (rc != AM_HEAD_OK && rc != AM_HEAD_BAIL)
        die("bad request result", data, len);
    if (rc == AM_HEAD_OK) {
        handled++;
        inside(rq.method, buf, len, data);
        inside(rq.path, buf, len, data);
        inside(rq.query, buf, len, data);
        inside(rq.content_type, buf, len, data);
        inside(rq.authorization, buf, len, data);
        if (rq.content_length < 0)
            die("negative content length", data, len);
        size_t pos = 0, pairs = 0;
        am_span name, value;
        while (am_query_next(rq.query.p, rq.query.n, &pos, &name, &value)) {
            inside(name, buf, len, data);
            inside(value, buf, len, data);
            if (value.n == 0 || ++pairs > rq.query.n)
                die("bad query pair", data, len);
        }
    }

    am_response_head rs;
    rc = am_parse_response_head(buf, len, &rs);
    if (rc != AM_HEAD_OK && rc != AM_HEAD_BAIL)
        die("bad response result", data, len);
    if (rc == AM_HEAD_OK) {
        handled++;
        if (rs.status < 0 || rs.status > 999 || rs.content_length < 0)
            die("bad response fields", data, len);
    }
    runs++;
    free(buf);
}

static const char *HEADS[] = {
    "GET /apis/activemonitor.keikoproj.io/v1alpha1/namespaces/health/healthchecks/hc-00001 HTTP/1.1\r\n"
    "Host: 127.0.0.1:40123\r\nContent-Type: application/json\r\nContent-Length: 0\r\n\r\n",
    "POST /apis/argoproj.io/v1alpha1/namespaces/health/workflows HTTP/1.1\r\n"
    "Host: localhost:8080\r\nContent-Type: application/json\r\n"
    "Authorization: Bearer s3cr3t\r\nContent-Length: 722\r\n\r\n",
    "GET /api/v1/pods?watch=true&allowWatchBookmarks=true&timeoutSeconds=300&&x=&y&=z&resourceVersion=4711 HTTP/1.1\r\n"
    "Host: h\r\nAccept: application/json;as=Table;v=v1\r\nExpect: 100-continue\r\n\r\n",
    "PUT /x HTTP/1.1\r\nContent-Length:  12 \r\nContent-Length: 13\r\nauthorization:   Bearer x  \r\n\r\n",
    "HTTP/1.1 200 OK\r\nContent-Type: application/json\r\nContent-Length: 722\r\n\r\n",
    "HTTP/1.1 401 Unauthorized\r\nContent-Type: application/json\r\n"
    "WWW-Authenticate: Bearer\r\nContent-Length: 104\r\n\r\n",
    "HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\nConnection: close\r\n\r\n",
    "HTTP/1.1 204\r\n\r\n",
};
#define NHEADS (sizeof(HEADS) / sizeof(HEADS[0]))

static const char REPLACEMENTS[] = {'\0', '\r', '\n', ':', ' ', (char)0xff};

/* xorshift64: the run is the same everywhere */
static unsigned long long rng_state = 0x9e3779b97f4a7c15ULL;

static unsigned long long
rng(void)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

int
main(void)
{
    /* every prefix, and every single byte replaced */
    for (size_t h = 0; h < NHEADS; h++) {
        size_t len = strlen(HEADS[h]);
        for (size_t i = 0; i <= len; i++)
            feed(HEADS[h], i);
        char *m = malloc(len);
        if (m == NULL)
            abort();
        for (size_t i = 0; i < len; i++) {
            for (size_t r = 0; r < sizeof(REPLACEMENTS); r++) {
                memcpy(m, HEADS[h], len);
                m[i] = REPLACEMENTS[r];
                feed(m, len);
            }
        }
        free(m);
    }
    if (handled == 0)
        die("no valid head was handled", "", 0);

    /* over-long values: target, header value, digits, header count */
    static const size_t SIZES[] = {17, 19, 64, 4096, 70000, 1 << 20};
    for (size_t s = 0; s < sizeof(SIZES) / sizeof(SIZES[0]); s++) {
        size_t n = SIZES[s];
        const char *fmt[][2] = {
            {"GET /", " HTTP/1.1\r\nHost: h\r\n\r\n"},
            {"GET /x?a=", " HTTP/1.1\r\n\r\n"},
            {"GET /x HTTP/1.1\r\nAuthorization: ", "\r\n\r\n"},
            {"GET /x HTTP/1.1\r\nContent-Length: ", "\r\n\r\n"},
            {"GET /x HTTP/1.1\r\nContent-Length:", "1\r\n\r\n"},
            {"HTTP/1.1 200 OK\r\nContent-Length: ", "\r\n\r\n"},
            {"HTTP/1.1 200 ", "\r\n\r\n"},
            {"", " /x HTTP/1.1\r\n\r\n"},
        };
        const char fill[] = {'a', 'a', 't', '9', ' ', '9', 'K', 'G'};
        for (size_t f = 0; f < sizeof(fmt) / sizeof(fmt[0]); f++) {
            size_t a = strlen(fmt[f][0]), b = strlen(fmt[f][1]);
            char *m = malloc(a + n + b);
            if (m == NULL)
                abort();
            memcpy(m, fmt[f][0], a);
            memset(m + a, fill[f], n);
            memcpy(m + a + n, fmt[f][1], b);
            feed(m, a + n + b);
            free(m);
        }
    }

    /* 10 000 seeded random byte strings: half raw bytes, half drawn from
     * the bytes heads are made of, so some get past the first line */
    static const char ALPHABET[] = "GET /?=&: \r\n\r\nHTTP/1.1 200 content-length:0123456789aZ%+";
    char m[512];
    for (int i = 0; i < 10000; i++) {
        size_t len = (size_t)(rng() % sizeof(m));
        for (size_t k = 0; k < len; k++) {
            unsigned long long r = rng();
            m[k] = (i & 1) ? ALPHABET[r % (sizeof(ALPHABET) - 1)] : (char)(r & 0xff);
        }
        feed(m, len);
    }
    printf("check_head: %lu inputs, %lu handled, no report\n", runs, handled);
    return 0;
}
