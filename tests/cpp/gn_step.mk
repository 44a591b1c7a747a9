# tests/cpp/test_gn_step: the one Gauss-Newton step under the single and the batched alignment
# loops (form_amd/csrc/align_host.hpp and refine_host.hpp, no HIP headers), plain g++ -Werror
# like its neighbours, with the address and undefined-behaviour sanitizers (runtimes linked
# statically: the program needs nothing preloaded).  -ffp-contract=off: pose.hpp's rounding, as
# the library builds it.
# Built by __graft_entry__.build():  make -C tests/cpp -f gn_step.mk
CXX ?= g++
ROOT := ../..
CXXFLAGS ?= -O1 -g -std=c++17 -ffp-contract=off -Wall -Wextra -Werror -fsanitize=address,undefined \
	-fno-sanitize-recover=all -static-libasan -static-libubsan
all: test_gn_step
test_gn_step: test_gn_step.cpp $(ROOT)/form_amd/csrc/refine_host.hpp $(ROOT)/form_amd/csrc/score_host.hpp \
		$(ROOT)/form_amd/csrc/align_host.hpp $(ROOT)/form_amd/csrc/nearest_host.hpp $(ROOT)/form_amd/csrc/probe_host.hpp \
		$(ROOT)/form_amd/csrc/carve_host.hpp $(ROOT)/form_amd/csrc/pose.hpp $(ROOT)/include/fmx/fmx.h
	$(CXX) $(CXXFLAGS) -I$(ROOT)/form_amd/csrc -I$(ROOT)/include -o $@ test_gn_step.cpp
clean:
	rm -f test_gn_step
.PHONY: all clean
