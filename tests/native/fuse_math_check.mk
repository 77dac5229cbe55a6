# The elevation arithmetic of rsp_beam_elev_dev on the host (tests/test_fuse_cpu.py builds and runs both):
# plain, and with the address and undefined-behaviour sanitizers.  A makefile of its own, run from this
# directory with `make -f fuse_math_check.mk OUT=<dir>`; OUT is where the two programs go.
OUT ?= build
CSRC := ../../radar-signal-process_amd/csrc
FLAGS := -std=c++17 -O2 -ffp-contract=off -Wall -Werror -I$(CSRC)
DEPS := fuse_math_check.cpp $(CSRC)/rsp_fuse_math.h $(CSRC)/rsp_measure_math.h

all: $(OUT)/fuse_math_check $(OUT)/fuse_math_check_san

$(OUT)/fuse_math_check: $(DEPS)
	mkdir -p $(OUT)
	g++ $(FLAGS) fuse_math_check.cpp -o $@

$(OUT)/fuse_math_check_san: $(DEPS)
	mkdir -p $(OUT)
	g++ $(FLAGS) -g -fsanitize=address,undefined -fno-sanitize-recover=all fuse_math_check.cpp -o $@

.PHONY: all
