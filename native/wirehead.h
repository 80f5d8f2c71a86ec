/* wirehead: HTTP/1.1 head parsing for the wire path, free of the Python API.
 *
 * Both parsers take one complete head (up to and including the terminating
 * CRLF CRLF) and answer either AM_HEAD_OK with a filled struct or
 * AM_HEAD_BAIL ("not handled"). They never guess: every input whose exact
 * answer needs the general Python code bails, and the caller runs that code.
 * The structs only point into the caller's buffer; nothing is allocated.
 *
 * native/_amcore.c wraps them for CPython; native/check/check_head.c links
 * this file alone and runs it under the sanitizers.
 */
#ifndef AM_WIREHEAD_H
#define AM_WIREHEAD_H

#include <stddef.h>

#define AM_HEAD_OK 0
#define AM_HEAD_BAIL 1

#define AM_FLAG_EXPECT_CONTINUE 1
#define AM_FLAG_WANT_TABLE 2

typedef struct {
    const char *p;
    size_t n;
} am_span;

typedef struct {
    am_span method;
    am_span path;
    am_span query;          /* the part after the first '?', may be empty */
    long long content_length;
    am_span content_type;   /* stripped value, empty when absent */
    am_span authorization;  /* stripped value, empty when absent */
    int flags;
} am_request_head;

typedef struct {
    int status;
    long long content_length;
    int chunked;
    int keep_alive;
} am_response_head;

int am_parse_request_head(const char *buf, size_t len, am_request_head *out);
int am_parse_response_head(const char *buf, size_t len, am_response_head *out);

/* Iterate the name=value pairs of a query string the way
 * urllib.parse.parse_qsl does with its defaults: pieces are separated by
 * '&'; a piece without '=' or with an empty value is dropped. *pos starts
 * at 0; returns 1 with name/value filled, 0 at the end. */
int am_query_next(const char *q, size_t len, size_t *pos,
                  am_span *name, am_span *value);

#endif
