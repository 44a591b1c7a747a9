# tests/cpp/test_scan_check: the scan-and-pose checks the dense map's calls share
# (form_amd/csrc/probe_host.hpp, no HIP headers), plain g++ -Werror like its neighbours, with
# the address and undefined-behaviour sanitizers (runtimes linked statically: the program needs
# nothing preloaded).
# Built by __graft_entry__.build():  make -C tests/cpp -f scan_check.mk
CXX ?= g++
ROOT := ../..
CXXFLAGS ?= -O1 -g -std=c++17 -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all \
	-static-libasan -static-libubsan
all: test_scan_check
test_scan_check: test_scan_check.cpp $(ROOT)/form_amd/csrc/probe_host.hpp $(ROOT)/form_amd/csrc/carve_host.hpp \
		$(ROOT)/include/fmx/fmx.h
	$(CXX) $(CXXFLAGS) -I$(ROOT)/form_amd/csrc -I$(ROOT)/include -o $@ test_scan_check.cpp
clean:
	rm -f test_scan_check
.PHONY: all clean
