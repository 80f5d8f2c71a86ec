# Developer entry points (parity with the reference Makefile's test/build/run
# targets, adapted to the Python stack).
PY ?= python3

.PHONY: test test-gpu bench run manifests native native-check docker-build sweep soak e2e-kind lint

test:
	$(PY) -m pytest tests/ -q -m "not gpu"

test-gpu:
	$(PY) -m pytest tests/ -q -m gpu

bench:
	$(PY) bench.py --steps 10 --warmup 2

sweep:
	$(PY) benchmarks/worker_sweep.py

run:
	$(PY) -m active_monitor_amd.cmd.main --backend memory --max-workers 10

native:
	$(PY) setup.py build_ext --inplace

# Memory-safety check of the C code, CPU only: two stand-alone programs built
# with the sanitizers (native/check/). check_head links the Python-free head
# parsers; check_json is an interpreter with the extension compiled in, run
# on the JSON corpus of tests/unit/test_wirecodec_json.py. The extension is
# never loaded under a sanitizer from inside `python`.
SANITIZE = -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	-fno-omit-frame-pointer -g -O1 -Wall -Wextra -Inative

native-check:
	$(CC) $(SANITIZE) -o native/check/check_head \
		native/check/check_head.c native/wirehead.c
	native/check/check_head
	$(CC) $(SANITIZE) -Wno-unused-parameter $$($(PY)-config --includes) \
		-o native/check/check_json native/check/check_json.c \
		native/_amcore.c native/wirejson.c native/wirehead.c \
		$$($(PY)-config --embed --ldflags)
	ASAN_OPTIONS=detect_leaks=0 native/check/check_json native/check/check_json.py

manifests:
	$(PY) -m active_monitor_amd.api.crd > config/crd/bases/activemonitor.keikoproj.io_healthchecks.yaml

docker-build:
	docker build -t active-monitor-amd:latest .

soak:
	$(PY) benchmarks/soak.py --crs 1000 --repeat 5 --duration 300

e2e-kind:
	hack/e2e-kind.sh

lint:
	ruff check --select E9,F63,F7,F82 .
